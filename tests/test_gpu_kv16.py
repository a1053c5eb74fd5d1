"""GPU: the half-precision key / value cache -- npm_kv_append_f16, npm_kv_gather_f16, npm_mha_decode_fwd_f16 (csrc/npm_decode.hip)
through the C ABI, then MultiHeadAttention / TransformerDecoder with ``dtype='f16'`` caches.

What is held to what:
* an append stores NumPy's ``astype(np.float16)`` BIT FOR BIT (uint16 equality, the edge row of tests/kv16_reference.py included);
  a gather returns the stored halves exactly, zeros at and past a length;
* the fp16 attention equals the fp32 entry point of the same layout on a cache holding the rounded values BITWISE, ctx and lse
  (tests/kv16_reference.py ``bitwise_cases``: every head size, row block count, length around the tile, split mode, load policy,
  batch and layout), and so inherits that kernel's float64 bounds (tests/decode_gpu.py ``check``, unchanged);
* the layers: float64 attention over the rows AS STORED (taken from ``cache.gather`` after each call) at tests/test_gpu_decode.py's
  LAYER_TOL; chunked decoding against one call at 2 LAYER_TOL;
* the distance to the fp32 cache: the derived worst case of tests/kv16_reference.py ``derived_bound`` (the fraction used is printed).

Every test names an ``_f16`` entry point, ``dtype=`` or ``cache_dtype=``: none exists without the feature.
"""

import ctypes as C

import numpy as np
import pytest

import attn_range_data as R
import decode_cases as DC
import decode_gpu
import decode_reference as DR
import kv16_reference as K16
import varlen_reference as VR
from decode_gpu import GUARD, NT_KNOB, SENTINEL
from kv16_reference import NAN16, SENTINEL16

pytestmark = pytest.mark.gpu

LAYER_TOL = 1e-5                  # tests/test_gpu_decode.py: float32 attention + projections at O(1) activations against float64
BAD_ARGUMENT, UNSUPPORTED = 10002, 10003


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.fixture(autouse=True)
def _defaults_afterwards(npm):
    yield
    decode_gpu.reset_knobs()


def _lib():
    from np_modeling_amd import _C
    return _C.lib()


def _append16(src, src_pitch, src_offset, cache, pitch, stride, batch, tokens, row_len, at=0, at_lens=None, new_lens=None, paged=None,
              cache_offset=0):
    """npm_kv_append_f16 of host rows ``src`` (float32, any shape: [batch * tokens, src_pitch] flat) into the device buffer ``cache``."""
    from np_modeling_amd import device as D
    sd = D.from_host(src)
    lens = None if at_lens is None else decode_gpu.ints(at_lens)
    new = None if new_lens is None else decode_gpu.ints(new_lens)
    table, table_pitch, page_rows = (None, 0, 0) if paged is None else (decode_gpu.ints(paged[0]), paged[0].shape[1], paged[1])
    return _lib().npm_kv_append_f16(sd.ptr + 4 * src_offset, src_pitch, cache.ptr + cache_offset, pitch, stride, batch, tokens, row_len, at,
                                    None if lens is None else lens.ptr, None if new is None else new.ptr,
                                    None if table is None else table.ptr, table_pitch, page_rows)


def _fill16(x, lens=None, paged=None, fill_bits=NAN16):
    """A device fp16 cache holding the rows of ``x`` [B, rows, Hkv, D] (float32 host), written by npm_kv_append_f16: contiguous
    [B, rows, Hkv * D], or with ``paged = (table, page_rows)`` a pool; only rows below ``lens[b]`` (None: all) are written, every
    other half -- and the guard region -- holds ``fill_bits``.  Returns (buffer, halves, pitch, stride)."""
    from np_modeling_amd import _C
    b, rows, hkv, d = x.shape
    row = hkv * d
    if paged is None:
        buf, n = K16.half_buffer([b, rows, row], fill_bits)
        stride = rows * row
        if lens is None:
            rc = _append16(x, row, 0, buf, row, stride, b, rows, row)
        else:
            rc = _append16(x, row, 0, buf, row, stride, b, rows, row, at_lens=np.zeros(b, dtype=np.int32), new_lens=lens)
    else:
        table, page_rows = paged
        pages = int(table.max()) + 3
        buf, n = K16.half_buffer([pages, page_rows, row], fill_bits)
        stride = page_rows * row
        rc = _append16(x, row, 0, buf, row, stride, b, rows, row, at_lens=np.zeros(b, dtype=np.int32),
                       new_lens=np.full(b, rows, dtype=np.int32) if lens is None else lens, paged=paged)
    _C.check(rc, 'npm_kv_append_f16')
    return buf, n, row, stride


def _bits(buf, n, fill_bits):
    bits = buf.numpy().view(np.uint16)
    np.testing.assert_array_equal(bits[n:], fill_bits)                    # the guard region
    return bits[:n]


def _decode16(q, kbuf, vbuf, pitch, stride, hkv, lmax, scale, causal, kv_lens=None, new_lens=None, paged=None, expect=0, k_offset=0,
              null_lens=False):
    """npm_mha_decode_fwd_f16 -> ctx [B, T, Hq, D], lse [B, Hq, T], kernel string.  ``expect``: the call must return that code and
    leave ctx and lse at their sentinels."""
    from np_modeling_amd import _C, device as D
    b, t, hq, d = q.shape
    qd = D.from_host(q)
    ctx = D.full([b * t * hq * d + GUARD], SENTINEL)
    lse = D.full([b * hq * t + GUARD], SENTINEL)
    c = _C.npm_mha_decode()
    c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim = b, hq, hkv, t, lmax, d
    c.causal, c.scale = int(causal), scale
    c.q, c.q_pitch = qd.ptr, hq * d
    c.k, c.k_pitch, c.k_stride_b = kbuf.ptr + k_offset, pitch, stride
    c.v, c.v_pitch, c.v_stride_b = vbuf.ptr, pitch, stride
    c.ctx, c.ctx_pitch, c.lse = ctx.ptr, hq * d, lse.ptr
    lens = None if kv_lens is None or null_lens else decode_gpu.ints(kv_lens)
    new = None if new_lens is None else decode_gpu.ints(new_lens)
    table, table_pitch, page_rows = (None, 0, 0) if paged is None else (decode_gpu.ints(paged[0]), paged[0].shape[1], paged[1])
    rc = _lib().npm_mha_decode_fwd_f16(C.byref(c), None if lens is None else lens.ptr, None if new is None else new.ptr,
                                       None if table is None else table.ptr, table_pitch, page_rows)
    if expect:
        assert rc == expect, (rc, _lib().npm_last_error())
        assert b'npm_mha_decode_fwd_f16:' in _lib().npm_last_error(), 'the error names the entry point that was called'
        np.testing.assert_array_equal(ctx.numpy(), SENTINEL)
        np.testing.assert_array_equal(lse.numpy(), SENTINEL)
        return None
    _C.check(rc, 'npm_mha_decode_fwd_f16')
    return (decode_gpu.guarded(ctx, b * t * hq * d).reshape(b, t, hq, d), decode_gpu.guarded(lse, b * hq * t).reshape(b, hq, t),
            _C.last_decode_kernel())


# ---- 1. append: NumPy's rounding, bit for bit ---------------------------------------------------------------------------------------
def _packed_source(rng, b, t, hq, hkv, d, scale=1.0):
    """K rows inside a packed [B, T, Hq + 2 Hkv, D] projection whose other columns are NaN: (buffer, pitch, offset, rows)."""
    pitch, offset, row = (hq + 2 * hkv) * d, hq * d, hkv * d
    src = np.full([b * t, pitch], np.nan, dtype=np.float32)
    rows = (rng.standard_normal([b * t, row]) * scale).astype(np.float32)
    rows[0, :K16.EDGE_VALUES.size] = K16.EDGE_VALUES
    src[:, offset:offset + row] = rows
    return src, pitch, offset, rows


@pytest.mark.parametrize('d,hkv', [(16, 1), (16, 3), (128, 1), (128, 3)])
@pytest.mark.parametrize('at', [0, 5])
def test_append_uniform_is_numpy_rounding_bit_for_bit(npm, d, hkv, at):
    from np_modeling_amd import _C
    rng = np.random.default_rng(d + hkv + at)
    b, t, cap, row = 3, 7, 14, hkv * d
    src, pitch, offset, rows = _packed_source(rng, b, t, 4, hkv, d, scale=40.0)
    buf, n = K16.half_buffer([b, cap, row])
    _C.check(_append16(src, pitch, offset, buf, row, cap * row, b, t, row, at=at), 'npm_kv_append_f16')
    got = _bits(buf, n, SENTINEL16).reshape(b, cap, row)
    want = np.full([b, cap, row], SENTINEL16, dtype=np.uint16)
    want[:, at:at + t] = K16.to_f16(rows).view(np.uint16).reshape(b, t, row)
    assert np.array_equal(got, want)
    assert np.array_equal(got[0, at, :K16.EDGE_BITS.size], K16.EDGE_BITS)          # inf at 65520, ties to even, subnormals, -0


@pytest.mark.parametrize('d,hkv', [(16, 3), (128, 1)])
@pytest.mark.parametrize('layout', ['varlen', 'paged16', 'paged64'])
def test_append_per_sequence_is_numpy_rounding_bit_for_bit(npm, d, hkv, layout):
    from np_modeling_amd import _C
    rng = np.random.default_rng(d + len(layout))
    b, t, cap, row = 3, 9, 80, hkv * d
    at, new = np.array([5, 17, 63], dtype=np.int32), np.array([9, 0, 4], dtype=np.int32)       # one sequence brings nothing
    src, pitch, offset, rows = _packed_source(rng, b, t, 4, hkv, d, scale=1e-3)
    want16 = K16.to_f16(rows).view(np.uint16).reshape(b, t, row)
    if layout == 'varlen':
        buf, n = K16.half_buffer([b, cap, row])
        _C.check(_append16(src, pitch, offset, buf, row, cap * row, b, t, row, at=3, at_lens=at, new_lens=new), 'npm_kv_append_f16')
        want = np.full([b, cap, row], SENTINEL16, dtype=np.uint16)
        for i in range(b):
            want[i, at[i]:at[i] + new[i]] = want16[i, :new[i]]
    else:
        page_rows = int(layout[5:])
        table, pages = K16.paged_table(rng, b, cap, page_rows)
        buf, n = K16.half_buffer([pages, page_rows, row])
        _C.check(_append16(src, pitch, offset, buf, row, page_rows * row, b, t, row, at_lens=at, new_lens=new, paged=(table, page_rows)),
                 'npm_kv_append_f16')
        want = np.full([pages, page_rows, row], SENTINEL16, dtype=np.uint16)
        for i in range(b):
            for j in range(new[i]):
                want[table[i, (at[i] + j) // page_rows], (at[i] + j) % page_rows] = want16[i, j]
    assert np.array_equal(_bits(buf, n, SENTINEL16).reshape(want.shape), want)


# ---- 2. gather: exact, zeros at and past the length ---------------------------------------------------------------------------------
@pytest.mark.parametrize('d,hkv', [(16, 3), (128, 1), (64, 2)])
@pytest.mark.parametrize('layout', ['contiguous', 'paged16', 'paged64'])
def test_gather_is_exact_and_reads_nothing_past_a_length(npm, d, hkv, layout):
    from np_modeling_amd import _C, device as D
    rng = np.random.default_rng(d + hkv)
    b, cap, rows, row = 3, 70, 66, hkv * d
    lens = np.array([66, 0, 33], dtype=np.int32)
    stored = rng.integers(0, 0x7c00, size=[b, cap, row]).astype(np.uint16) | (rng.integers(0, 2, size=[b, cap, row]).astype(np.uint16) << 15)
    stored[0, 0, :K16.EDGE_BITS.size] = K16.EDGE_BITS                     # inf, subnormals, -0 come back exactly
    for i in range(b):
        stored[i, lens[i]:] = NAN16                                       # rows past the length: NaN, never read
    out = D.full([b * rows * row + GUARD], SENTINEL)
    if layout == 'contiguous':
        buf, dev_lens = K16.upload_halves(stored), decode_gpu.ints(lens)
        rc = _lib().npm_kv_gather_f16(buf.ptr, row, cap * row, out.ptr, b, rows, row, dev_lens.ptr, None, 0, 0)
    else:
        page_rows = int(layout[5:])
        table, pages = K16.paged_table(rng, b, cap, page_rows)
        pool = K16.to_pages(stored, table, page_rows, pages, fill=NAN16)
        for i in range(b):
            table[i, -(-int(lens[i]) // page_rows):] = -1                 # entries past the last page are not read
        buf, tab, dev_lens = K16.upload_halves(pool), decode_gpu.ints(table), decode_gpu.ints(lens)
        rc = _lib().npm_kv_gather_f16(buf.ptr, row, page_rows * row, out.ptr, b, rows, row, dev_lens.ptr, tab.ptr, table.shape[1], page_rows)
    _C.check(rc, 'npm_kv_gather_f16')
    got = decode_gpu.guarded(out, b * rows * row).reshape(b, rows, row)
    want = np.zeros([b, rows, row], dtype=np.float32)
    for i in range(b):
        want[i, :lens[i]] = stored[i, :lens[i]].view(np.float16).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 3. / 4. the fp16 kernel against the fp32 kernel on the rounded values (bitwise) and against float64 ---------------------------------
def _lengths(b, t, length, layout):
    """(kv_lens, new_lens) of a case: the uniform call has none; the others include a sequence without rows and a padded token."""
    if layout == 'uniform':
        return None, None
    if b == 1:
        return np.array([length], dtype=np.int32), np.array([max(t - 1, 1)], dtype=np.int32)
    third = max(length - 3, 1)
    return np.array([length, 0, third], dtype=np.int32), np.array([t, 0, min(max(t - 1, 1), third)], dtype=np.int32)


def _both(q, k, v, length, scale, causal, layout, kv_lens, new_lens, seed):
    """The fp16 call on a cache filled by npm_kv_append_f16 and the fp32 call of the same layout on the rounded values."""
    b = q.shape[0]
    hkv = k.shape[2]
    k32, v32 = K16.rounded(k), K16.rounded(v)
    valid = np.full(b, length, dtype=np.int32) if kv_lens is None else kv_lens
    for i in range(b):                                                    # nothing past a length may matter, in either cache
        k32[i, valid[i]:], v32[i, valid[i]:] = np.nan, np.nan
    if layout.startswith('paged'):
        page_rows = int(layout[5:])
        table, pages = K16.paged_table(np.random.default_rng(seed), b, k.shape[1], page_rows, spare=3)
        paged = (table, page_rows)
        kbuf, n, pitch, stride = _fill16(k, valid, paged)
        vbuf = _fill16(v, valid, paged)[0]
        got = _decode16(q, kbuf, vbuf, pitch, stride, hkv, length, scale, causal, kv_lens, new_lens, paged)
        want = decode_gpu.run(q, K16.to_pages(k32, table, page_rows, int(table.max()) + 3, np.nan),
                              K16.to_pages(v32, table, page_rows, int(table.max()) + 3, np.nan), length, scale, causal, kv_lens, new_lens,
                              paged=paged)
    else:
        kbuf, n, pitch, stride = _fill16(k, valid)                        # rows at and past a length keep their NaN
        vbuf = _fill16(v, valid)[0]
        got = _decode16(q, kbuf, vbuf, pitch, stride, hkv, length, scale, causal, kv_lens, new_lens)
        want = decode_gpu.run(q, k32, v32, length, scale, causal, kv_lens, new_lens)
    _bits(kbuf, n, NAN16)                                                 # the guard region behind the cache
    return got, want, (k32, v32)


@pytest.mark.parametrize('case', K16.bitwise_cases(), ids=K16.case_id)
def test_f16_kernel_equals_the_f32_kernel_on_the_rounded_values_bitwise(npm, case):
    from np_modeling_amd import _C
    d, hq, hkv, t, length, causal, mode, nt, b, layout = case
    q, k, v = decode_gpu.data(d * 7 + hq + t + length + causal, b, t, hq, hkv, d, length + 5)
    kv_lens, new_lens = _lengths(b, t, length, layout)
    scale = 1.0 / np.sqrt(d)
    _C.check(_C.lib().npm_set_tuning(NT_KNOB, nt), 'npm_set_tuning')
    forced = decode_gpu.set_splits(mode, length)
    splits = forced or _C.lib().npm_mha_decode_splits(b, hkv, length)
    (ctx, lse, kernel), (ctx32, lse32, kernel32), (k32, v32) = _both(q, k, v, length, scale, causal, layout, kv_lens, new_lens, seed=length + d)
    tail = {'uniform': '', 'varlen': ' varlen=1', 'paged16': ' varlen=1 paged=16', 'paged64': ' varlen=1 paged=64'}[layout]
    assert kernel32 == f'mha_decode_kernel D={d} rows={hq // hkv * t} splits={splits} causal={causal}{tail}'
    assert kernel == kernel32 + ' kv=f16'
    assert np.array_equal(ctx.view(np.uint32), ctx32.view(np.uint32)), f'{kernel}: ctx differs from the fp32 kernel on the rounded values'
    assert np.array_equal(lse.view(np.uint32), lse32.view(np.uint32)), f'{kernel}: lse differs from the fp32 kernel on the rounded values'
    # 4. float64 of the rounded values, at the fp32 kernel's own bounds
    lens = np.full(b, length) if kv_lens is None else kv_lens
    new = np.full(b, t) if new_lens is None else new_lens
    decode_gpu.check(ctx, lse, q, np.nan_to_num(k32), np.nan_to_num(v32), lens, new, scale, causal, kernel + f' L={length} B={b}')


# ---- 5. repeats and neighbours ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,hq,hkv,t,length,mode', [(128, 8, 2, 1, 529, 'auto'), (64, 8, 8, 4, 300, 3), (16, 6, 3, 2, 100, 'one'),
                                                    (32, 8, 1, 4, 17, 'many')])
def test_repeats_layouts_and_poison_are_bitwise_neutral(npm, d, hq, hkv, t, length, mode):
    b, cap = 3, length + 40
    q, k, v = decode_gpu.data(31 + d, b, t, hq, hkv, d, cap)
    scale, lens = 1.0 / np.sqrt(d), np.full(b, length, dtype=np.int32)

    def run(fill_bits, layout, kv_lens=None, qq=q, new_lens=None):
        decode_gpu.set_splits(mode, length)
        paged = None
        if layout.startswith('paged'):
            page_rows = int(layout[5:])
            paged = (K16.paged_table(np.random.default_rng(5), b, cap, page_rows)[0], page_rows)
        kbuf, n, pitch, stride = _fill16(k, lens, paged, fill_bits)
        vbuf = _fill16(v, lens, paged, fill_bits)[0]
        return _decode16(qq, kbuf, vbuf, pitch, stride, hkv, length, scale, 1, kv_lens, new_lens, paged)

    base = run(0x0000, 'contiguous')
    again = run(0x0000, 'contiguous')
    assert np.array_equal(base[0], again[0]) and np.array_equal(base[1], again[1]) and base[2] == again[2]        # the same call twice
    for fill in (NAN16, K16.INF16):                                       # poisoned rows past L never matter
        other = run(fill, 'contiguous')
        assert np.isfinite(other[0]).all() and np.array_equal(base[0], other[0]) and np.array_equal(base[1], other[1])
    varlen = run(NAN16, 'contiguous', lens)                               # all lengths equal: the varlen call is the uniform call
    assert np.array_equal(base[0], varlen[0]) and np.array_equal(base[1], varlen[1]) and varlen[2].endswith('varlen=1 kv=f16')
    for layout in ('paged16', 'paged64'):                                 # paged equals contiguous
        paged = run(NAN16, layout, lens)
        assert np.array_equal(varlen[0], paged[0]) and np.array_equal(varlen[1], paged[1]) and paged[2].endswith(f'paged={layout[5:]} kv=f16')
    if t > 1:                                                             # NaN query padding: rows t >= n[b] are zeros, the others unchanged
        new = np.array([t, t - 1, 1], dtype=np.int32)
        clean = run(NAN16, 'contiguous', lens, new_lens=new)
        qp = q.copy()
        qp[np.arange(t)[None, :] >= new[:, None]] = np.nan
        dirty = run(NAN16, 'contiguous', lens, qq=qp, new_lens=new)
        assert np.isfinite(dirty[0]).all() and np.array_equal(clean[0], dirty[0]) and np.array_equal(clean[1], dirty[1])
        assert (dirty[0][np.arange(t)[None, :] >= new[:, None]] == 0).all()


# ---- 6. refusals: the documented code, nothing launched, nothing written ------------------------------------------------------------
def test_refused_calls_return_the_documented_code_and_write_nothing(npm):
    from np_modeling_amd import device as D
    rng = np.random.default_rng(3)
    b, cap, hkv, d, hq, t = 2, 32, 2, 16, 4, 2
    row = hkv * d
    q, k, v = decode_gpu.data(1, b, t, hq, hkv, d, cap)
    kbuf, n, pitch, stride = _fill16(k, None, None, SENTINEL16)
    vbuf = _fill16(v, None, None, SENTINEL16)[0]
    table = np.arange(4, dtype=np.int32).reshape(2, 2)
    lens = np.full(b, cap, dtype=np.int32)
    ok = _decode16(q, kbuf, vbuf, pitch, stride, hkv, cap, 0.25, 1)
    assert ok[2].endswith('kv=f16')
    # the attention
    _decode16(q, kbuf, vbuf, row + 4, stride, hkv, cap, 0.25, 1, expect=BAD_ARGUMENT)                     # a pitch of 4 halves past the row
    _decode16(q, kbuf, vbuf, pitch, stride + 4, hkv, cap, 0.25, 1, expect=BAD_ARGUMENT)
    _decode16(q, kbuf, vbuf, pitch, stride, hkv, cap, 0.25, 1, k_offset=8, expect=BAD_ARGUMENT)           # the pointer off by 8 bytes
    _decode16(q, kbuf, vbuf, pitch, 16 * row, hkv, cap, 0.25, 1, None, None, (table, 16), expect=BAD_ARGUMENT)    # a table without lengths
    _decode16(q, kbuf, vbuf, pitch, 8 * row, hkv, cap, 0.25, 1, lens, None, (np.arange(8, dtype=np.int32).reshape(2, 4), 8),
              expect=BAD_ARGUMENT)                                                                        # page_rows 8
    _decode16(q, kbuf, vbuf, pitch, stride, hkv, t - 1, 0.25, 1, expect=BAD_ARGUMENT)                     # kv_len < new_tokens, uniform
    q48 = rng.standard_normal([b, t, 2, 48]).astype(np.float32)
    _decode16(q48, kbuf, vbuf, 48, 4 * 48, 1, 4, 0.25, 1, expect=UNSUPPORTED)                             # head size 48
    q33 = rng.standard_normal([b, 1, 66, 16]).astype(np.float32)
    _decode16(q33, kbuf, vbuf, pitch, stride, 2, cap, 0.25, 0, expect=UNSUPPORTED)                        # 33 group rows
    # the append
    src = rng.standard_normal([b * t, row]).astype(np.float32)
    fresh, m = K16.half_buffer([b, cap, row])
    for kwargs, what in ((dict(pitch=row + 4), 'pitch'), (dict(stride=cap * row + 4), 'stride'), (dict(cache_offset=8), 'pointer'),
                         (dict(row_len=12), 'row_len 12'), (dict(paged=(table, 16)), 'a table without lengths'),
                         (dict(paged=(table, 8), at_lens=np.zeros(b, dtype=np.int32)), 'page_rows 8')):
        args = dict(pitch=row, stride=cap * row, row_len=row)
        args.update(kwargs)
        pitch_, stride_, row_len = args.pop('pitch'), args.pop('stride'), args.pop('row_len')
        assert _append16(src, row, 0, fresh, pitch_, stride_, b, t, row_len, **args) == BAD_ARGUMENT, what
    assert (_bits(fresh, m, SENTINEL16) == SENTINEL16).all()              # the cache keeps its sentinel
    # the gather
    out = D.full([b * 4 * row + GUARD], SENTINEL)
    dev_lens, tab = decode_gpu.ints(lens), decode_gpu.ints(table)
    lib = _lib()
    assert lib.npm_kv_gather_f16(kbuf.ptr, row + 4, stride, out.ptr, b, 4, row, dev_lens.ptr, None, 0, 0) == BAD_ARGUMENT
    assert lib.npm_kv_gather_f16(kbuf.ptr + 8, row, stride, out.ptr, b, 4, row, dev_lens.ptr, None, 0, 0) == BAD_ARGUMENT
    assert lib.npm_kv_gather_f16(kbuf.ptr, row, stride, out.ptr, b, 4, 12, dev_lens.ptr, None, 0, 0) == BAD_ARGUMENT
    assert lib.npm_kv_gather_f16(kbuf.ptr, row, 16 * row, out.ptr, b, 4, row, None, tab.ptr, 2, 16) == BAD_ARGUMENT
    assert lib.npm_kv_gather_f16(kbuf.ptr, row, 8 * row, out.ptr, b, 4, row, dev_lens.ptr, tab.ptr, 2, 8) == BAD_ARGUMENT
    np.testing.assert_array_equal(out.numpy(), SENTINEL)


# ---- 7. MultiHeadAttention over an fp16 cache ----------------------------------------------------------------------------------------
def _stored_step(p, x, cache, n):
    """float64 attention of the chunk ``x`` [B, T, F] (sequence b brings n[b] tokens, already appended) over the rows AS STORED."""
    k, v = (np.asarray(r, dtype=np.float64) for r in cache.gather(max(cache.max_length, 1)))
    q = DR._project(np.asarray(x, dtype=np.float64), p['wq'], p['bq'])
    ctx, _ = VR.decode_attention(q, k, v, cache.lengths, n, 1.0 / np.sqrt(q.shape[3]), True)
    return np.einsum('...abc,...dbc->...ad', ctx, p['wo']) + p['bo']


def _run_plan(att, p, cache, plan, f, seed, expect_paths):
    rng = np.random.default_rng(seed)
    b = cache.batch
    for step, (t, n, release) in enumerate(plan):
        if release is not None:
            cache.release(release)
        x = rng.standard_normal([b, t, f]).astype(np.float32)
        got = np.asarray(att(x, cache=cache, new_lengths=n))
        assert att._cached_path == expect_paths[step], (step, att._cached_path)
        n = np.full(b, t) if n is None else np.asarray(n)
        want = _stored_step(p, x, cache, n)
        for i in range(b):
            if n[i]:
                decode_gpu.layer_close(got[i, :n[i]], want[i, :n[i]], LAYER_TOL, f'step {step} T={t} sequence {i} ({att._cached_path})')


@pytest.mark.parametrize('heads,kv_heads', [(8, 8), (8, 2)])
@pytest.mark.parametrize('d', [16, 64])
@pytest.mark.parametrize('kind', ['contiguous', 'ragged', 'paged'])
def test_layer_over_an_f16_cache_against_float64_of_the_stored_rows(npm, heads, kv_heads, d, kind):
    f = heads * d
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads + d, batch=3)
    if kind == 'contiguous':
        cache = att.make_cache(3, 60, dtype='f16')
        plan = [(40, None, None), (1, None, None), (3, None, None), (1, None, None)]
        paths = ['fused_masked', 'decode', 'decode', 'decode']
    elif kind == 'ragged':
        cache = att.make_cache(3, 60, dtype='f16')
        plan = [(40, [40, 7, 0], None), (1, [1, 1, 1], None), (3, [3, 0, 2], None), (1, None, None)]
        paths = ['fused_masked', 'decode', 'decode', 'decode']
    else:
        cache = att.make_cache(3, 96, page_size=16, dtype='f16')
        plan = [(40, [40, 7, 20], None), (1, None, None), (3, [1, 3, 0], 1), (40, [2, 40, 1], None), (1, None, None)]
        paths = ['fused_masked', 'decode', 'decode', 'fused_masked', 'decode']
    assert cache.dtype == 'f16' and cache.nbytes == cache.k.nbytes * 2
    _run_plan(att, p, cache, plan, f, seed=d, expect_paths=paths)
    stored = np.asarray(cache.gather(cache.max_length)[0])
    assert np.array_equal(stored, K16.rounded(stored))                    # what the cache holds are halves


def test_layer_cross_attention_prefill_switch_and_split_math(npm):
    from np_modeling_amd import _C, device as D
    att, p = DC.make_mha(npm, 256, 8, 2, seed=3, batch=3)
    rng = np.random.default_rng(8)
    kv = rng.standard_normal([3, 50, 256]).astype(np.float32)
    cache = att.fill_cache(att.make_cache(3, 64, dtype='f16'), kv)
    k, v = (np.asarray(r, dtype=np.float64) for r in cache.gather(50))
    for t in (1, 4, 70):
        x = rng.standard_normal([3, t, 256]).astype(np.float32)
        got = np.asarray(att(x, cache=cache))
        assert att._cached_path == ('decode' if t <= 8 else 'fused_masked')
        want = DR.mha_cross_cached(p, x, dict(k=k, v=v))
        decode_gpu.layer_close(got, want, LAYER_TOL, f'cross over an f16 cache T={t}')
    # the prefill switch changes nothing for an fp16 cache: the same calls, bitwise
    x = rng.standard_normal([3, 45, 256]).astype(np.float32)
    outs = []
    saved = D.PREFILL_KERNEL
    try:
        for switch in (False, True):
            D.PREFILL_KERNEL = switch
            own = att.make_cache(3, 64, dtype='f16')
            outs.append([np.asarray(att(np.ascontiguousarray(piece), cache=own)) for piece in DC.split(x, [40, 1, 4])])
            assert att._cached_path == 'decode'
    finally:
        D.PREFILL_KERNEL = saved
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    _C.set_math('bf16x3')
    try:
        own = att.make_cache(3, 64, dtype='f16')
        out = np.asarray(att(x[:, :3], cache=own))
        assert att._cached_path == 'fused_masked' and np.isfinite(out).all()
    finally:
        _C.set_math('f32')


# ---- 8. TransformerDecoder ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('page_size', [None, 16])
def test_decoder_chunked_decoding_with_f16_caches(npm, page_size):
    f, steps = 64, 8
    dec, _ = DC.make_decoder(npm, f, 4, 2, 96, True, True, seed=11, batch=2, seq_kv=7)
    rng = np.random.default_rng(12)
    q, kv = rng.standard_normal([2, steps, f]).astype(np.float32), rng.standard_normal([2, 7, f]).astype(np.float32)
    kwargs = {} if page_size is None else dict(page_size=page_size)
    state = dec.start_decoding(kv, 24, cache_dtype='f16', **kwargs)
    plain = dec.start_decoding(kv, 24, **kwargs)
    assert state.self_cache.dtype == state.cross_cache.dtype == 'f16' and plain.self_cache.dtype == 'f32'
    assert 2 * state.self_cache.nbytes == plain.self_cache.nbytes and 2 * state.cross_cache.nbytes == plain.cross_cache.nbytes
    got = np.concatenate([np.asarray(dec.decode(np.ascontiguousarray(q[:, i:i + 1]), state)) for i in range(steps)], axis=1)
    assert state.position == steps
    whole = np.asarray(dec.decode(q, dec.start_decoding(kv, 24, cache_dtype='f16', **kwargs)))
    decode_gpu.layer_close(got, whole, 2 * LAYER_TOL, f'token by token vs one call, f16 caches, page_size {page_size}')
    ref = np.asarray(dec.decode(q, plain))
    print('f16 caches vs fp32 caches: max |difference| %.3e (reported; test 9 bounds the attention itself)' % float(np.abs(whole - ref).max()))


# ---- 9. the distance to the fp32 cache ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [16, 64, 128])
def test_distance_to_the_f32_cache_stays_within_the_derived_bound(npm, d):
    """|ctx16 - ctx32| <= (expm1(2 eps) + u) max|v| + the fp32 kernel's bound on either side, eps = u scale max sum_i |q_i| |k_i|
    (tests/kv16_reference.py ``derived_bound``): a worst case derived from the format, not a measurement.  N(0, 1) data."""
    D = npm.device
    b, hq, hkv, t, length = 3, 8, 2, 2, 529
    q, k, v = decode_gpu.data(90 + d, b, t, hq, hkv, d, length)
    scale = 1.0 / np.sqrt(d)
    ctx = {}
    for dtype in ('f32', 'f16'):
        cache = D.KVCache(b, length + 3, hkv, d, dtype=dtype)
        cache.append(D.Mat(D.from_host(k), hkv * d), D.Mat(D.from_host(v), hkv * d), length)
        ctx[dtype] = np.asarray(cache.attend(D.Mat(D.from_host(q), hq * d), hq, t, scale, True)[0]).astype(np.float64)
    want, want_lse = DR.decode_attention(q, k, v, length, scale, True)
    x = R.exponent_magnitude(q, k, scale, want_lse)
    kernel_bound = 2 * R.exponent_tol(2e-6, x) * (1.0 + float(np.abs(want).max()))
    bound, eps = K16.derived_bound(q, k, v, scale, kernel_bound)
    used = float(np.abs(ctx['f16'] - ctx['f32']).max() / bound)
    print(f'D={d} L={length}: eps {eps:.3e}, max |ctx16 - ctx32| {np.abs(ctx["f16"] - ctx["f32"]).max():.3e}, '
          f'{100 * used:.2f} % of the derived bound {bound:.3e}')
    assert 0 < used <= 1.0
