"""GPU: every grid-stride copy kernel past its first trip, through the C ABI, with no tolerance.

The kernels that move rows into, out of and between KV caches loop over a flat work index, and every other call of the suite is
smaller than their grid: a wrong stride, a ``return`` where ``continue`` is meant or a decode that holds only for i < lanes would pass
it.  Here every call makes at least two trips with a partial last one (tests/stride_cases.py has the shapes and the arithmetic,
tests/test_stride_host.py proves them on the CPU and checks the expectations imported here).  Whole buffers are compared as raw
bits -- row padding, untouched rows and pages, and a guard region of sentinels behind each buffer.

a. npm_rope_kv_append (against npm_rope and the appends at the default grid), npm_cvt_f32_f16 / npm_cvt_f16_f32 and npm_take_rows
   (against NumPy) under NPM_TUNE_EW_GRID_CAP 1 / 2 / 3, each call only at the caps at which it loops.
b. npm_kv_append, _varlen, _paged, _f16 and npm_kv_gather_varlen, _paged, _f16 at 545 280 items over 2048 x 256 lanes.
c. npm_kv_copy_pages / npm_kv_copy_pages_planes past 16 384 pieces, 65 535 pairs and 65 535 planes.
d. npm_rope and npm_rope_kv_append refuse 2^31 items with NPM_E_UNSUPPORTED and write nothing.
"""

import numpy as np
import pytest

import stride_cases as SC
import test_gpu_rope_append as RA

pytestmark = pytest.mark.gpu

BITS = {2: np.uint16, 4: np.uint32}


@pytest.fixture(scope='module')
def env():
    from np_modeling_amd import _C, device
    return _C.lib(), device


class capped:
    """``with capped(n):`` -- NPM_TUNE_EW_GRID_CAP n for the block, the library's default (knob value 0) afterwards."""

    def __init__(self, cap):
        self.cap = cap

    def _set(self, value):
        from np_modeling_amd import _C
        _C.check(_C.lib().npm_set_tuning(SC.KNOB_EW_GRID_CAP, value), 'npm_set_tuning')

    def __enter__(self):
        self._set(self.cap)

    def __exit__(self, *exc):
        self._set(0)
        return False


@pytest.fixture(autouse=True)
def _cap_back():
    try:
        yield
    finally:
        capped(0)._set(0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(BITS[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def _read(buf, dtype):
    return buf.numpy().view(dtype)


def _same(got, want, what):
    """Raw bits; where a mismatch is, for the message."""
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        raise AssertionError(f'{what}: {bad.size} of {g.size} elements differ, the first at {bad[0]}, the last at {bad[-1]}: '
                             f'got {got.ravel()[bad[:4]]} want {want.ravel()[bad[:4]]}')


# ---- a. under the grid cap ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap', SC.EW_CAPS)
@pytest.mark.parametrize('d', [64, 12])
def test_rope_kv_append_loops_leave_the_bits_of_the_three_launches(env, d, cap):
    """The yardstick -- npm_rope, then the append of the layout for the k and the v heads -- runs at the default grid, where no lane
    loops; the fused call runs under the cap.  Packed buffer, K pool and V pool as raw bits, and the instance's name."""
    lib, D = env
    assert (RA.B, RA.STARTS, RA.CAP, RA.PAGE) == (SC.ROPE_B, SC.ROPE_STARTS, SC.ROPE_TABLE_ROWS, 16)
    ran = 0
    for c in SC.rope_cases():
        if c.d != d or not SC.rope_loops(c, cap):
            continue
        lens = None if c.mode == 'scalar' else np.array(SC.ROPE_NEW_LENS)
        case = RA.Case(D, c.d, c.heads, c.kv_heads, SC.ROPE_T, c.mode, c.f16, c.rope, True, lens, SC.ROPE_PAD, c.tight)
        assert case.table_rows == (max(SC.ROPE_STARTS) + 2 if c.tight else SC.ROPE_TABLE_ROWS) and case.vec == (d == 64)
        x_ref, k_ref, v_ref = case.fresh()
        x_got, k_got, v_got = case.fresh()
        assert case.three_launches(lib, x_ref, k_ref, v_ref) == 0, (c, lib.npm_last_error())
        with capped(cap):
            rc = case.fused(lib, x_got, k_got, v_got)
        assert rc == 0, (c, cap, lib.npm_last_error())
        assert lib.npm_last_rope_append_kernel().decode() == case.name(), (c, cap)
        what = f'{c} cap {cap} ({SC.rope_total(c)} items over {SC.ew_lanes(SC.rope_total(c), cap)} lanes)'
        _same(x_got.numpy(), x_ref.numpy(), what + ': the packed buffer')
        dtype = np.float16 if c.f16 else np.float32
        _same(_read(k_got, dtype), _read(k_ref, dtype), what + ': the K pool')
        _same(_read(v_got, dtype), _read(v_ref, dtype), what + ': the V pool')
        assert not np.array_equal(_read(k_ref, dtype), case.pool0) and (_read(k_ref, dtype)[-RA.GUARD:] == RA.SENTINEL).all(), what
        ran += 1
    print(f'D{d} cap {cap}: {ran} looping calls')
    assert ran >= (32 if cap == 1 else 26)


def _nan_aware(got, want, what):
    """The special set holds one NaN twice: NaN where NaN is expected, raw bits everywhere else."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ': NaN positions'
    _same(np.where(nan, 0, got).astype(got.dtype), np.where(nan, 0, want).astype(want.dtype), what)


@pytest.mark.parametrize('shape', SC.CVT_SHAPES, ids=lambda s: f'{s[0]}cols')
def test_conversion_loops_round_and_widen_exactly(env, shape):
    lib, D = env
    cols, p32, p16 = shape
    case = SC.cvt_case(shape)
    total = SC.CVT_ROWS * SC.cvt_per_row(*shape)
    ran = 0
    for cap in SC.EW_CAPS:
        if not SC.loops(total, SC.ew_lanes(total, cap)):
            continue
        src32, dst16 = D.from_host(case['src32']), D.bytes_from_host(np.full_like(case['want16'], SC.SENTINEL))
        src16, dst32 = D.bytes_from_host(case['src16']), D.from_host(np.full_like(case['want32'], SC.SENTINEL))
        with capped(cap):
            assert lib.npm_cvt_f32_f16(src32.ptr, p32, dst16.ptr, p16, SC.CVT_ROWS, cols) == 0, lib.npm_last_error()
            assert lib.npm_cvt_f16_f32(src16.ptr, p16, dst32.ptr, p32, SC.CVT_ROWS, cols) == 0, lib.npm_last_error()
        _nan_aware(_read(dst16, np.float16), case['want16'], f'f32 -> f16 {shape} cap {cap}')
        _nan_aware(dst32.numpy(), case['want32'], f'f16 -> f32 {shape} cap {cap}')
        ran += 1
    assert ran == (1 if cols == 72 else 3)


@pytest.mark.parametrize('shape', SC.TAKE_SHAPES, ids=lambda s: f'{s[0]}cols')
def test_row_lookup_loops_copy_rows_and_zero_the_outside_ones(env, shape):
    lib, D = env
    cols, sp, dp = shape
    case = SC.take_case(shape)
    total = SC.TAKE_ROWS * SC.take_per_row(*shape)
    src, idx = D.from_host(case['src']), D.bytes_from_host(case['idx'])
    ran = 0
    for cap in SC.EW_CAPS:
        if not SC.loops(total, SC.ew_lanes(total, cap)):
            continue
        dst = D.from_host(np.full_like(case['want'], SC.SENTINEL))
        with capped(cap):
            assert lib.npm_take_rows(src.ptr, sp, SC.TAKE_SRC_ROWS, idx.ptr, dst.ptr, dp, SC.TAKE_ROWS, cols) == 0, lib.npm_last_error()
        _same(dst.numpy(), case['want'], f'take_rows {shape} cap {cap}')
        ran += 1
    assert ran == (2 if cols == 100 else 3)


# ---- b. the row copies --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lengths(env):
    """at_lens, new_lens / lens and the block tables of both cache types on the device, once."""
    _, D = env
    out = {}
    for kv in ('f32', 'f16'):
        out[kv] = dict(at=D.bytes_from_host(SC.row_at_lens(kv)), n=D.bytes_from_host(SC.row_lens(kv)),
                       table=D.bytes_from_host(SC.row_tables(kv)[0]))
    return out


@pytest.mark.parametrize('kv,layout,source', SC.APPEND_CASES, ids=lambda v: str(v))
def test_appends_past_the_grid_store_every_row_and_nothing_else(env, lengths, kv, layout, source):
    lib, D = env
    case = SC.append_case(kv, layout, source)
    src, cache = D.from_host(case['src']), D.bytes_from_host(case['cache0'])
    from_, pitch, cp, stride = src.ptr + 4 * case['offset'], case['pitch'], SC.ROW_CACHE_PITCH, case['stride']
    dev = lengths[kv]
    paging = (dev['table'].ptr, SC.ROW_CACHE_ROWS[kv] // SC.ROW_PAGE, SC.ROW_PAGE) if layout == 'paged' else (None, 0, 0)
    b, t, n = SC.ROW_B, SC.ROW_T[kv], SC.ROW_LEN
    if kv == 'f16':
        ragged = (0, dev['at'].ptr, dev['n'].ptr) if layout != 'uniform' else (SC.ROW_AT, None, None)
        rc = lib.npm_kv_append_f16(from_, pitch, cache.ptr, cp, stride, b, t, n, *ragged, *paging)
    elif layout == 'paged':
        rc = lib.npm_kv_append_paged(from_, pitch, cache.ptr, cp, stride, b, t, n, dev['at'].ptr, dev['n'].ptr, *paging)
    elif layout == 'varlen':
        rc = lib.npm_kv_append_varlen(from_, pitch, cache.ptr, cp, stride, b, t, n, dev['at'].ptr, dev['n'].ptr)
    else:
        rc = lib.npm_kv_append(from_, pitch, cache.ptr, cp, stride, b, t, n, SC.ROW_AT)
    assert rc == 0, lib.npm_last_error()
    _same(_read(cache, SC.ROW_DTYPE[kv]), case['want'], f'append {kv} {layout} {source}')


@pytest.mark.parametrize('kv,layout', SC.GATHER_CASES, ids=lambda v: str(v))
def test_gathers_past_the_grid_copy_the_valid_rows_and_zero_the_rest(env, kv, layout):
    lib, D = env
    case = SC.gather_case(kv, layout)
    cache, out, lens = D.bytes_from_host(case['cache']), D.from_host(case['out0']), D.bytes_from_host(case['lens'])
    cp, stride, b, t, n = SC.ROW_CACHE_PITCH, case['stride'], SC.ROW_B, SC.ROW_T[kv], SC.ROW_LEN
    table = D.bytes_from_host(case['table']) if layout == 'paged' else None
    paging = (table.ptr, SC.ROW_CACHE_ROWS[kv] // SC.ROW_PAGE, SC.ROW_PAGE) if layout == 'paged' else (None, 0, 0)
    if kv == 'f16':
        rc = lib.npm_kv_gather_f16(cache.ptr, cp, stride, out.ptr, b, t, n, lens.ptr, *paging)
    elif layout == 'paged':
        rc = lib.npm_kv_gather_paged(cache.ptr, cp, stride, out.ptr, b, t, n, lens.ptr, *paging)
    else:
        rc = lib.npm_kv_gather_varlen(cache.ptr, cp, stride, out.ptr, b, t, n, lens.ptr)
    assert rc == 0, lib.npm_last_error()
    _same(out.numpy(), case['want'], f'gather {kv} {layout}')
    _same(_read(cache, SC.ROW_DTYPE[kv]), case['cache'], f'gather {kv} {layout}: the cache')


# ---- c. the page copies -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c.name for c in SC.PAGE_CASES])
def test_page_copies_past_the_end_of_a_grid_dimension(env, name):
    lib, D = env
    built = SC.page_case(name)
    c = built['case']
    pairs = D.bytes_from_host(np.concatenate([built['src'], built['dst'], built['rows']]).astype(np.int32))
    src, dst, rows = pairs.ptr, pairs.ptr + 4 * c.n, pairs.ptr + 8 * c.n
    pool = D.bytes_from_host(built['pool0'])
    assert lib.npm_kv_copy_pages_planes(pool.ptr, c.page_bytes, c.row_bytes, src, dst, rows, c.n, c.planes, c.plane_bytes) == 0, \
        lib.npm_last_error()
    _same(_read(pool, np.uint32), built['want'], f'{name}: npm_kv_copy_pages_planes')
    if name.startswith(('pieces', 'pairs')):                        # one plane: npm_kv_copy_pages, which leaves the others alone
        pool = D.bytes_from_host(built['pool0'])
        assert lib.npm_kv_copy_pages(pool.ptr, c.page_bytes, c.row_bytes, src, dst, rows, c.n) == 0, lib.npm_last_error()
        _same(_read(pool, np.uint32), SC.page_case(name, planes=1)['want'], f'{name}: npm_kv_copy_pages')


# ---- d. the 32-bit index refusal ----------------------------------------------------------------------------------------------------
def test_two_to_the_31_items_are_refused_and_nothing_is_written(env):
    """Exactly one item more than the kernels' unsigned 32-bit loop can count: NPM_E_UNSUPPORTED before any launch.  The buffers are
    small and real; a launch would have to write them."""
    lib, D = env
    b, t, d = SC.REFUSE_BATCH, SC.REFUSE_TOKENS, SC.REFUSE_D
    zeros = np.zeros(t * d // 2, dtype=np.float32)
    cos, sin = D.from_host(zeros + 1), D.from_host(zeros)
    host = np.full(8192, SC.SENTINEL, dtype=np.float32)
    x = D.from_host(host)
    assert x.ptr % 16 == 0 and cos.ptr % 16 == 0 and sin.ptr % 16 == 0                  # the vector instance: 16 items per head
    assert lib.npm_rope(x.ptr, SC.REFUSE_HEADS * d, b, t, SC.REFUSE_HEADS, d, cos.ptr, sin.ptr, t, 0, None, 0) == SC.UNSUPPORTED
    assert '2147483648 work items' in lib.npm_last_error().decode()
    _same(x.numpy(), host, 'npm_rope')
    for kind, heads, kv_heads in SC.REFUSE_APPEND:
        for f16 in (0, 1):
            k, v = D.from_host(host), D.from_host(host)
            tables = (cos.ptr, sin.ptr, t) if kind == 'rope' else (None, None, 0)
            rc = lib.npm_rope_kv_append(x.ptr, (heads + 2 * kv_heads) * d, b, t, heads, kv_heads, d, *tables, 0, None, None, k.ptr, v.ptr,
                                        kv_heads * d, t * kv_heads * d, None, 0, 0, f16)
            assert rc == SC.UNSUPPORTED, (kind, f16, rc, lib.npm_last_error())
            assert '2147483648 work items' in lib.npm_last_error().decode()
            for buf, what in ((x, 'qkv'), (k, 'K'), (v, 'V')):
                _same(buf.numpy(), host, f'npm_rope_kv_append {kind} f16={f16}: {what}')
