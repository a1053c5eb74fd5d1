"""CPU: the shapes of tests/stride_cases.py do what tests/test_gpu_stride.py needs them to do -- every call makes at least two trips of
its kernel's grid-stride loop, the last trip is partial, and the rows that the loop body skips, stores and decodes into different
sequences lie behind the first trip -- and the NumPy expectations hold together: sentinels and guards where nothing is written,
zeros behind a length in a gather.  Conditions on shapes, recomputed from the launch code; nothing here is measured."""

import numpy as np
import pytest

import stride_cases as SC


def _bytes(*arrays):
    return max(a.nbytes for a in arrays)


# ---- a. under the grid cap ----------------------------------------------------------------------------------------------------------
def test_the_lane_counts_are_those_of_the_launch_code():
    assert [SC.ew_lanes(1200, cap) for cap in SC.EW_CAPS] == [256, 512, 768]
    assert SC.ew_lanes(480, 2) == 512 and SC.ew_lanes(480, 3) == 512 and SC.ew_lanes(1, 3) == 256 and SC.ew_lanes(0, 1) == 256
    assert SC.row_copy_lanes(537600) == 524288 and SC.row_copy_lanes(524288) == 524288 and SC.row_copy_lanes(1000) == 1024
    assert SC.trips(1200, 768) == 2 and SC.trips(768, 768) == 1 and SC.loops(1200, 768) and not SC.loops(1536, 768)


def test_rope_append_item_counts_are_the_stated_ones():
    totals = {(c.d, c.heads, c.rope): SC.rope_total(c) for c in SC.rope_cases()}
    assert totals[64, 6, True] == 1200 and totals[64, 6, False] == 480 and totals[12, 6, True] == 900 and totals[12, 6, False] == 360
    assert totals[64, 8, True] == 2880 and totals[64, 8, False] == 1920 and totals[12, 8, True] == 2160 and totals[12, 8, False] == 1440
    cases = SC.rope_cases()
    assert len(cases) == len(set(cases)) == 2 * 2 * (12 + 4)
    # scalar-at / varlen / paged x f32 / f16 x rope / cos == NULL, and the tight table for varlen and paged, at both head sizes
    for shape in SC.ROPE_SHAPES:
        for d in (64, 12):
            mine = [c for c in cases if (c.heads, c.kv_heads) == shape and c.d == d]
            assert {(c.mode, c.f16, c.rope) for c in mine if not c.tight} == {(m, f, r) for m in ('scalar', 'varlen', 'paged')
                                                                              for f in (False, True) for r in (False, True)}
            assert {(c.mode, c.f16, c.rope) for c in mine if c.tight} == {(m, f, True) for m in ('varlen', 'paged') for f in (False, True)}
            assert (shape[1] * d) % 8 == 0                                   # an fp16 cache row of whole 8-half steps: no call is refused


def test_without_tables_the_issue_shape_loops_at_cap_1_only():
    """480 and 360 items are below 512: caps 2 and 3 give two blocks and one trip.  The GPU test runs a case only where it loops."""
    for c in SC.rope_cases():
        looping = [cap for cap in SC.EW_CAPS if SC.rope_loops(c, cap)]
        assert looping == ([1, 2, 3] if c.rope or c.heads == 8 else [1]), c


@pytest.mark.parametrize('cap', SC.EW_CAPS)
def test_rope_append_tails_hold_skipped_stored_and_off_table_rows_of_two_sequences(cap):
    checked = 0
    for c in SC.rope_cases():
        if not SC.rope_loops(c, cap):
            continue
        f = SC.rope_facts(c, cap)
        assert f['trips'] >= 2 and f['partial'] and f['total'] % f['lanes'] != 0, (c, f)
        checked += 1
        if c.mode == 'scalar':                                               # no per-sequence skip: every row is stored
            assert not f['skipped'] and f['stored'] and not f['idle'], (c, f)
            continue
        thin = SC.ROPE_THIN_TAILS.get((c.rope, cap)) if (c.d, c.heads) == (12, 6) else None
        if thin is None:
            assert f['skipped'] and f['stored'] and f['sequences'] >= 2, (c, f)
            assert f['idle'], (c, f)
        else:                                                                # what the docstring of ROPE_THIN_TAILS works out
            assert f['skipped'] and f['sequences'] == thin['sequences'] and f['stored'] == thin['stored'], (c, f)
            twin = c._replace(heads=8, kv_heads=8)
            g = SC.rope_facts(twin, cap)
            assert SC.rope_loops(twin, cap) and g['skipped'] and g['stored'] and g['sequences'] >= 2, (twin, g)
        if c.tight:
            assert f['off_table'], (c, f)
        else:
            assert not f['off_table'], (c, f)
    assert checked >= 40


def test_in_every_ragged_rope_append_instance_a_lane_that_took_the_continue_works_again_on_a_later_trip():
    """What a ``return`` in place of the ``continue`` would break.  Not at every cap (at cap 1 of the 480-item call the lanes that
    idle on trip 1 idle on trip 2 as well), but for every instance -- head size, layout, cache type, with and without tables --
    at one cap at least."""
    resumes = {}
    for c in SC.rope_cases():
        if c.mode != 'scalar':
            key = (c.d, c.mode, c.f16, c.rope, c.tight)
            resumes[key] = resumes.get(key, False) or any(SC.rope_loops(c, cap) and SC.rope_facts(c, cap)['resumes'] for cap in SC.EW_CAPS)
    assert len(resumes) == 2 * 2 * 2 * 3 and all(resumes.values()), resumes


def test_rope_append_buffers_are_small():
    for c in SC.rope_cases():
        width = (c.heads + 2 * c.kv_heads) * c.d
        assert 4 * (SC.ROPE_B * SC.ROPE_T * (width + SC.ROPE_PAD)) < SC.NT_BYTES and 4 * 10 * 16 * c.kv_heads * c.d < SC.NT_BYTES


@pytest.mark.parametrize('shape', SC.CVT_SHAPES)
def test_conversion_cases(shape):
    cols, p32, p16 = shape
    per_row = SC.cvt_per_row(*shape)
    assert per_row == {72: 9, 45: 45, 184: 23}[cols] and SC.CVT_ROWS * per_row == {72: 333, 45: 1665, 184: 851}[cols]
    assert p32 > cols and p16 > cols and (cols != 45 or (p32 % 2 and p16 % 2))
    total = SC.CVT_ROWS * per_row
    looping = [cap for cap in SC.EW_CAPS if SC.loops(total, SC.ew_lanes(total, cap))]
    assert looping == ([1] if cols == 72 else [1, 2, 3])                      # 333 items are below 512
    case = SC.cvt_case(shape)
    assert _bytes(*[v for v in case.values() if isinstance(v, np.ndarray)]) < SC.NT_BYTES
    # the special values at the end lie behind the first trip of every looping cap
    w = cols // per_row
    assert all(case['first_special'] // w >= SC.ew_lanes(total, cap) for cap in looping)
    for want, src, pitch in ((case['want16'], case['src32'], p16), (case['want32'], case['src16'], p32)):
        body = want[:-SC.GUARD].reshape(SC.CVT_ROWS, pitch)
        assert (want[-SC.GUARD:] == SC.SENTINEL).all() and (body[:, cols:] == SC.SENTINEL).all()
        from_ = src[:-SC.GUARD].reshape(SC.CVT_ROWS, -1)[:, :cols]
        nan = np.isnan(from_)
        assert nan.sum() == 2 and np.array_equal(np.isnan(body[:, :cols]), nan)
        with np.errstate(over='ignore'):
            assert np.array_equal(body[:, :cols][~nan], from_[~nan].astype(body.dtype))
        assert np.isinf(body[:, :cols]).sum() == 14                          # the seven of the special set from 65520 up, twice


@pytest.mark.parametrize('shape', SC.TAKE_SHAPES)
def test_row_lookup_cases(shape):
    cols, sp, dp = shape
    per_row = SC.take_per_row(*shape)
    total = SC.TAKE_ROWS * per_row
    assert total == {100: 575, 99: 2277, 136: 782}[cols] and sp > cols and dp > cols
    looping = [cap for cap in SC.EW_CAPS if SC.loops(total, SC.ew_lanes(total, cap))]
    assert looping == ([1, 2] if cols == 100 else [1, 2, 3])                  # 575 items are below 768
    idx = SC.TAKE_IDX
    assert len(idx) == SC.TAKE_ROWS and -1 in idx and SC.TAKE_SRC_ROWS in idx and len(set(idx)) < len(idx)
    for cap in looping:
        assert SC.take_rows_outside_in_tail(shape, cap), (shape, cap)
    case = SC.take_case(shape)
    body = case['want'][:-SC.GUARD].reshape(SC.TAKE_ROWS, dp)
    assert (case['want'][-SC.GUARD:] == SC.SENTINEL).all() and (body[:, cols:] == SC.SENTINEL).all()
    src = case['src'].reshape(SC.TAKE_SRC_ROWS, sp)
    for r, from_ in enumerate(idx):
        assert np.array_equal(body[r, :cols], src[from_, :cols] if 0 <= from_ < SC.TAKE_SRC_ROWS else np.zeros(cols, dtype=np.float32))
    assert not (src == 0).any() and not (src == SC.SENTINEL).any()


# ---- b. the row copies --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kv', ['f32', 'f16'])
def test_row_copy_shapes_put_zero_partial_and_full_sequences_behind_the_first_trip(kv):
    f = SC.row_facts(kv)
    t = SC.ROW_T[kv]
    assert f['total'] == 545280 and f['lanes'] == SC.ROW_COPY_GRID * SC.BLOCK == 524288 and f['trips'] == 2 and f['partial']
    assert f['sequences'] == [68, 69, 70] and f['tail_lens'] == [t, 0, t // 2 - 2] and SC.row_lens(kv)[67] == t
    assert f['first_tail_row'] == (68, {'f32': 8, 'f16': 16}[kv])             # trip 2 starts inside sequence 68
    assert f['skipped'] and f['stored'] and f['resumes']
    assert 0 < f['tail_lens'][2] < t
    uniform = SC.row_facts(kv, ragged=False)                                  # npm_kv_append has no lengths: every row is stored
    assert uniform['trips'] == 2 and uniform['partial'] and uniform['stored'] and not uniform['skipped']
    at = SC.row_at_lens(kv)
    assert len(set(at.tolist())) > 5 and at.min() >= 0 and (at + t <= SC.ROW_CACHE_ROWS[kv]).all() and SC.ROW_AT > 0
    assert SC.ROW_AT + t <= SC.ROW_CACHE_ROWS[kv] and SC.ROW_CACHE_ROWS[kv] % SC.ROW_PAGE == 0
    # the issue's B 70 cannot hold the three kinds of length in its tail: two sequences only
    total70 = 70 * t * (SC.ROW_LEN // SC.ROW_W[kv])
    assert total70 == 537600 and (total70 - 524288) // (SC.ROW_LEN // SC.ROW_W[kv]) == {'f32': 52, 'f16': 104}[kv] < 2 * t


@pytest.mark.parametrize('kv,layout,source', SC.APPEND_CASES)
def test_append_expectations(kv, layout, source):
    case = SC.append_case(kv, layout, source)
    t, pitch = SC.ROW_T[kv], SC.ROW_CACHE_PITCH
    assert _bytes(case['src'], case['cache0'], case['want']) < SC.NT_BYTES
    assert case['pitch'] > SC.ROW_LEN and (case['offset'] > 0) == (source == 'packed') and case['offset'] + SC.ROW_LEN <= case['pitch']
    assert case['pitch'] % 4 == 0 and case['offset'] % 4 == 0 and pitch % SC.ROW_W[kv] == 0 and case['stride'] % SC.ROW_W[kv] == 0
    want, cache0 = case['want'], case['cache0']
    assert (cache0 == SC.SENTINEL).all() and (want[-SC.GUARD:] == SC.SENTINEL).all()
    rows = want[:-SC.GUARD].reshape(-1, pitch)
    assert (rows[:, SC.ROW_LEN:] == SC.SENTINEL).all()                          # the padding of every row
    written = (rows[:, :SC.ROW_LEN] != SC.SENTINEL).all(axis=1)
    untouched = (rows[:, :SC.ROW_LEN] == SC.SENTINEL).all(axis=1)
    assert (written | untouched).all() and written.sum() == case['stored_rows'] == int(case['new_lens'].sum())
    if layout == 'uniform':
        assert case['stored_rows'] == SC.ROW_B * t and (case['at_lens'] == SC.ROW_AT).all()
        assert written.reshape(SC.ROW_B, -1)[:, SC.ROW_AT:SC.ROW_AT + t].all()
    if layout == 'paged':
        table = case['table']
        pages = rows.shape[0] // SC.ROW_PAGE
        spare = sorted(set(range(pages)) - set(table.ravel().tolist()))
        assert len(spare) == SC.ROW_SPARE_PAGES and len(set(table.ravel().tolist())) == table.size
        assert not written.reshape(pages, SC.ROW_PAGE)[spare].any()
        assert not np.array_equal(np.sort(table.ravel()), table.ravel())    # shuffled
    # the last stored row of the last sequence, by hand
    b = SC.ROW_B - 1
    n, at = int(case['new_lens'][b]), int(case['at_lens'][b])
    j = at + n - 1
    row = (case['table'][b, j // SC.ROW_PAGE] * SC.ROW_PAGE + j % SC.ROW_PAGE) if layout == 'paged' else b * SC.ROW_CACHE_ROWS[kv] + j
    src = case['src'].reshape(-1, case['pitch'])[b * t + n - 1, case['offset']:case['offset'] + SC.ROW_LEN]
    assert np.array_equal(rows[row, :SC.ROW_LEN], src.astype(SC.ROW_DTYPE[kv]))


@pytest.mark.parametrize('kv,layout', SC.GATHER_CASES)
def test_gather_expectations_have_zeros_behind_every_length(kv, layout):
    case = SC.gather_case(kv, layout)
    t = SC.ROW_T[kv]
    assert _bytes(case['cache'], case['out0'], case['want']) < SC.NT_BYTES
    assert (case['out0'] == SC.SENTINEL).all() and (case['want'][-SC.GUARD:] == SC.SENTINEL).all()
    body = case['want'][:-SC.GUARD].reshape(SC.ROW_B, t, SC.ROW_LEN)
    assert (case['cache'] != 0).mean() > 0.99                                   # a row that is read shows
    for b, n in enumerate(case['lens']):
        assert (body[b, n:] == 0).all() and (body[b, :n] != 0).mean() > 0.99 if n else (body[b] == 0).all()
    assert case['lens'][69] == 0 and case['lens'][68] == t and 0 < case['lens'][70] < t
    if layout == 'paged':
        for b, n in enumerate(case['lens']):
            used = -(-int(n) // SC.ROW_PAGE)
            assert (case['table'][b, used:] == SC.ROW_OUTSIDE_PAGE).all() and (case['table'][b, :used] >= 0).all()
        assert (case['table'][69] == SC.ROW_OUTSIDE_PAGE).all()
        # row 3 of sequence 70 through its table, by hand
        pool = case['cache'].reshape(-1, SC.ROW_PAGE, SC.ROW_CACHE_PITCH)
        assert np.array_equal(body[70, 3], pool[case['table'][70, 0], 3, :SC.ROW_LEN].astype(np.float32))
    else:
        rows = case['cache'].reshape(SC.ROW_B, SC.ROW_CACHE_ROWS[kv], SC.ROW_CACHE_PITCH)
        assert np.array_equal(body[70, 3], rows[70, 3, :SC.ROW_LEN].astype(np.float32))


# ---- c. the page copies -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', SC.PAGE_CASES, ids=lambda c: c.name)
def test_page_copy_cases_pass_the_end_of_one_grid_dimension(case):
    tr = SC.page_trips(case)
    kind = case.name.split('-')[0]
    work, lanes = tr[kind]
    assert SC.trips(work, lanes) == 2 and work % lanes == {'pieces': 256, 'pairs': 5, 'planes': 3}[kind]
    assert lanes == {'pieces': SC.PAGE_COPY_X * SC.BLOCK, 'pairs': SC.PAGE_COPY_YZ, 'planes': SC.PAGE_COPY_YZ}[kind]
    src, dst, rows = SC.page_pairs(case.name)
    assert len(set(src.tolist()) | set(dst.tolist())) == 2 * case.n and max(src.max(), dst.max()) < case.pages
    assert (rows * case.row_bytes <= case.page_bytes).all() and case.plane_bytes >= case.pages * case.page_bytes
    row16 = case.row_bytes // 16
    if kind == 'pieces':
        pieces = rows * row16
        assert pieces.tolist() == [16640, 16380, 260, 0] and lanes == 16384     # trip 2: 256 pieces of pair 0, none of the others
    if kind == 'pairs':
        assert set(rows[:SC.PAGE_COPY_YZ].tolist()) == {0, 1} and rows[SC.PAGE_COPY_YZ:].tolist() == [1, 0, 1, 1, 0]
    built = SC.page_case(case.name)
    pool0, want = built['pool0'], built['want']
    assert pool0.nbytes < SC.NT_BYTES and np.array_equal(want[-SC.GUARD:], pool0[-SC.GUARD:])
    changed = np.flatnonzero(want != pool0)
    copied = int(rows.sum()) * case.row_bytes // 4 * case.planes
    assert 0.99 * copied <= changed.size <= copied                              # equal words by chance aside, exactly the copied ones
    # the last copied row of the last plane, by hand
    last = int(np.flatnonzero(rows)[-1])
    base = (case.planes - 1) * case.plane_bytes // 4
    r = (int(rows[last]) - 1) * case.row_bytes // 4
    to, from_ = base + int(dst[last]) * case.page_bytes // 4 + r, base + int(src[last]) * case.page_bytes // 4 + r
    assert np.array_equal(want[to:to + case.row_bytes // 4], pool0[from_:from_ + case.row_bytes // 4])
    first = SC.page_case(case.name, planes=1)['want']                           # npm_kv_copy_pages: the first plane only
    assert np.array_equal(first[case.plane_bytes // 4:], pool0[case.plane_bytes // 4:]) or case.planes == 1
    assert np.array_equal(first[:case.plane_bytes // 4], want[:case.plane_bytes // 4])


# ---- d. the refusal -----------------------------------------------------------------------------------------------------------------
def test_the_refused_calls_have_exactly_two_to_the_31_items():
    assert SC.refuse_total(SC.REFUSE_HEADS) == SC.INDEX_LIMIT == 0x7fffffff + 1
    for kind, heads, kv_heads in SC.REFUSE_APPEND:
        assert SC.refuse_total(heads + 2 * kv_heads if kind == 'rope' else 2 * kv_heads) == SC.INDEX_LIMIT
