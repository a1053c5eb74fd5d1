"""The grid-stride copy kernels past their first trip: the cases, the launch arithmetic restated and the NumPy expectations, shared by
tests/test_stride_host.py (CPU) and tests/test_gpu_stride.py.

Every kernel here is a loop ``for (i = lane; i < total; i += lanes)`` over a flat work index that it decodes into (row, head, piece)
or (sequence, token, piece).  A *trip* is one pass of that loop; ``lanes`` is grid x 256.  The suite's other files never make a lane
take a second trip in these kernels; the shapes below are the smallest that do, with a partial last trip, and with the rows that the
loop body skips (``continue``), stores and decodes into two sequences lying in the trips behind the first.

a. Under NPM_TUNE_EW_GRID_CAP 1 / 2 / 3 (256 / 512 / 768 lanes): npm_rope_kv_append, npm_cvt_f32_f16 / npm_cvt_f16_f32, npm_take_rows.
   A call loops at a cap only where total > cap x 256; ``*_loops`` say where, and nothing is claimed for the other caps.  The shapes
   of the first rows of ROPE_SHAPES / CVT_SHAPES / TAKE_SHAPES are small enough that some instances loop at cap 1 only (480 items
   without rope tables, 333 of the vector conversion, 575 of the vector lookup), and at D 12 the tail of (H, Hkv) = (6, 2) is one
   sequence (ROPE_THIN_TAILS).  A second shape of each kind -- (H, Hkv) = (8, 8); 184 columns; 136 columns -- loops at all three caps
   with the full mix of rows in its tail.
b. The row copies behind row_copy<KV> (fixed 2048 x 256 lanes): rows of 1024 floats, B 71, T 30 (fp32 cache, 4 floats per item) or
   T 60 (fp16 cache, 8 halves per item): 545 280 items, 20 992 of them in trip 2 -- the end of sequence 68 and all of 69 and 70.
   B 71 and not 70: with 70 sequences trip 2 covers two sequences only (68 and 69), and a length of 0, a partial and a full one
   cannot all lie inside it.
c. The page copies: pieces of a page past 64 x 256 lanes, pairs past 65 535, planes past 65 535.

All kernels are exact copies, roundings (``astype(np.float16)``) or rotations; expectations are plain NumPy indexing written from
include/npm_hip.h, whole buffers with row padding, untouched rows and a guard region of sentinels behind them.
"""

import functools
import itertools
from collections import namedtuple

import numpy as np

# ---- the launch code, restated ------------------------------------------------------------------------------------------------------
BLOCK = 256                   # every launch here: ``dim3(256)`` / ``block(256)`` and ``__launch_bounds__(256)``
KNOB_EW_GRID_CAP = 7          # include/npm_hip.h: ``NPM_TUNE_EW_GRID_CAP = 7``
EW_CAPS = (1, 2, 3)           # tests/rowops_reference.py EW_CAPS; knob value 0 restores the library's 2^20 (npm::set_ew_grid_cap)
ROW_COPY_GRID = 2048          # csrc/npm_decode.hip row_copy: ``grid((unsigned)std::min<long>((total + 255) / 256, 2048))``
PAGE_COPY_X = 64              # npm_kv_copy_pages[_planes]: ``std::min<long>((page16 + 255) / 256, 64)``
PAGE_COPY_YZ = 65535          # the same two lines: ``std::min(n, 65535)`` and ``std::min(planes, 65535)``
ROW_W = {'f32': 4, 'f16': 8}  # csrc/npm_decode.hip ``RowVec<KV>::W``: 16 bytes of the cache per item
NT_BYTES = 1 << 25            # tests/rowops_reference.py NT_BYTES: nothing here reaches the size that switches a policy
SENTINEL, GUARD = 777.0, 256  # 777 is exact in fp16 too
UNSUPPORTED = 10003           # include/npm_hip.h: ``NPM_E_UNSUPPORTED = 10003``
INDEX_LIMIT = 1 << 31         # npm_rope / npm_rope_kv_append: ``if (total > 0x7fffffffLL)``


def ew_lanes(total, cap):
    """npm_rowops.hip grid_for / npm_rope_append.hip: ``max(1, min((total + 255) / 256, cap))`` blocks of 256."""
    return max(1, min(-(-total // BLOCK), cap)) * BLOCK


def row_copy_lanes(total):
    return min(-(-total // BLOCK), ROW_COPY_GRID) * BLOCK


def trips(total, lanes):
    return -(-total // lanes)


def loops(total, lanes):
    """At least two trips and a partial last one."""
    return trips(total, lanes) >= 2 and total % lanes != 0


def _resumes(idle, lanes):
    """Whether some lane runs into the loop body's ``continue`` on one trip and has work on a later one."""
    seen = np.zeros(lanes, dtype=bool)
    for first in range(0, idle.size, lanes):
        part = idle[first:first + lanes]
        if (seen[:part.size] & ~part).any():
            return True
        seen[:part.size] |= part
    return False


# ---- a. npm_rope_kv_append ----------------------------------------------------------------------------------------------------------
ROPE_B, ROPE_T = 3, 5                       # tests/test_gpu_rope_append.py: B, and its larger T
ROPE_STARTS, ROPE_NEW_LENS = (14, 3, 31), (5, 0, 2)
ROPE_PAD, ROPE_TABLE_ROWS = 8, 48           # pitch = width + 8; test_gpu_rope_append.py CAP: a table that holds every position
ROPE_SHAPES = ((6, 2), (8, 8))              # (H, Hkv): the issue's shape, and the one that loops at every cap (module docstring)
RopeCase = namedtuple('RopeCase', 'd heads kv_heads mode f16 rope tight')


def rope_cases():
    """Scalar-at / varlen / paged x f32 / f16 x rope / cos == NULL at D 64 (vector instance) and D 12 (scalar instance), and for
    varlen and paged the tight table whose last two rows are the first two of the last chunk, so that its tail runs off."""
    out = []
    for (heads, kv_heads), d in itertools.product(ROPE_SHAPES, (64, 12)):
        for mode, f16, rope in itertools.product(('scalar', 'varlen', 'paged'), (False, True), (True, False)):
            out.append(RopeCase(d, heads, kv_heads, mode, f16, rope, False))
        for mode, f16 in itertools.product(('varlen', 'paged'), (False, True)):
            out.append(RopeCase(d, heads, kv_heads, mode, f16, True, True))
    return out


def rope_pieces(d):
    """Items per head: npm_rope_append.hip ``vec ? half / 4 : half``, vec = head_dim % 8 == 0 (pitch and pointers are aligned here)."""
    return d // 2 // 4 if d % 8 == 0 else d // 2


def rope_total(c):
    """``batch * tokens * active * (vec ? half / 4 : half)``, active = ``rot ? heads + 2 * kv_heads : 2 * kv_heads``."""
    return ROPE_B * ROPE_T * (c.heads + 2 * c.kv_heads if c.rope else 2 * c.kv_heads) * rope_pieces(c.d)


def rope_facts(c, cap):
    """rope_kv_append_kernel's decode of every item: dict total, lanes, trips, partial, and over the items of trips >= 2: skipped
    (a row t >= new_lens[b]), stored, sequences (how many), off_table (a position the table has no row for), idle (the ``continue``);
    resumes: a lane that took the ``continue`` has work on a later trip."""
    pieces, total = rope_pieces(c.d), rope_total(c)
    active, first_head = (c.heads + 2 * c.kv_heads, 0) if c.rope else (2 * c.kv_heads, c.heads)
    lanes = ew_lanes(total, cap)
    i = np.arange(total)
    rh = i // pieces
    row, head = rh // active, first_head + rh % active
    b, t = row // ROPE_T, row % ROPE_T
    ragged = c.mode != 'scalar'
    starts = np.array(ROPE_STARTS if ragged else (ROPE_STARTS[0],) * ROPE_B)
    table_rows = int(starts.max()) + 2 if c.tight else ROPE_TABLE_ROWS
    skipped = (t >= np.array(ROPE_NEW_LENS)[b]) if ragged else np.zeros(total, dtype=bool)
    stored = (head >= c.heads) & ~skipped
    off = starts[b] + t >= table_rows
    rotated = (head < c.heads + c.kv_heads) & ~off if c.rope else np.zeros(total, dtype=bool)
    idle = ~rotated & ~stored
    tail = i >= lanes
    return dict(total=total, lanes=lanes, trips=trips(total, lanes), partial=total % lanes != 0, skipped=bool((skipped & tail).any()),
                stored=bool((stored & tail).any()), sequences=len(set(b[tail].tolist())), off_table=bool((off & tail).any()),
                idle=bool((idle & tail).any()), resumes=_resumes(idle, lanes))


def rope_loops(c, cap):
    return loops(rope_total(c), ew_lanes(rope_total(c), cap))


# Where the issue's own shape (H, Hkv) = (6, 2) cannot put the whole mix of rows behind the first trip at D 12: (rope, cap) ->
# what the tail is.  With tables a row is 10 heads x 6 pairs = 60 items and 900 in all: at cap 3 (768 lanes) the tail starts inside
# row 12 and is rows t = 2, 3, 4 of sequence 2, all of them past new_lens[2] = 2 -- one sequence, nothing stored.  Without tables a
# row is 4 heads x 6 = 24 items and 360 in all: at cap 1 the tail starts inside row 10 and is sequence 2 alone.  The (8, 8) shape
# has the whole mix at the same caps, which tests/test_stride_host.py asserts next to this.
ROPE_THIN_TAILS = {(True, 3): dict(sequences=1, stored=False), (False, 1): dict(sequences=1, stored=True)}


# ---- a. npm_cvt_f32_f16 / npm_cvt_f16_f32 and npm_take_rows ---------------------------------------------------------------------------
CVT_ROWS = 37
# (columns, fp32 pitch, fp16 pitch): the vector instance (9 items per row, 333), the scalar one (odd pitches; 1665 items), and a
# vector shape of 23 items per row, 851 in all, which loops at caps 2 and 3 too
CVT_SHAPES = ((72, 80, 88), (45, 47, 51), (184, 192, 200))
TAKE_ROWS, TAKE_SRC_ROWS = 23, 11
# (columns, source pitch, destination pitch): vector (25 items per row, 575), scalar (2277), vector with 34 per row (782: cap 3 loops)
TAKE_SHAPES = ((100, 104, 108), (99, 101, 103), (136, 140, 144))
TAKE_IDX = (3, 3, 0, -1, 10, 7, 7, 7, 1, 11, 2, 5, 9, 4, 6, 8, 0, 10, 3, 2, 5, -1, 11)     # repeats; -1 and 11 are rows of zeros


def cvt_per_row(cols, f32_pitch, f16_pitch):
    """npm_rowops.hip cvt_launch: ``vec = cols % 8 == 0 && half_pitch % 8 == 0 && f32_pitch % 4 == 0`` (and 16-byte aligned
    pointers, which the buffers here have); ``per_row = vec ? cols / 8 : cols``."""
    return cols // 8 if cols % 8 == 0 and f16_pitch % 8 == 0 and f32_pitch % 4 == 0 else cols


def take_per_row(cols, src_pitch, dst_pitch):
    """npm_take_rows: ``vec = cols % 4 == 0 && src_pitch % 4 == 0 && dst_pitch % 4 == 0``; ``per_row = vec ? cols / 4 : cols``."""
    return cols // 4 if cols % 4 == 0 and src_pitch % 4 == 0 and dst_pitch % 4 == 0 else cols


def special_floats():
    """The set of tests/test_gpu_w16.py: ties at the half spacing, values whose halves are subnormal or flush to 0, +-65520 and
    its neighbours, +-inf, NaN."""
    ties = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -23, 2048.0 + 1.0, 2048.0 + 3.0,
            -(1 + 2.0 ** -11), 0.1, -0.1, 1 / 3, 1000.7, 3.14159265]
    sub = [2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -15, 3.0 * 2.0 ** -24, 2.5 * 2.0 ** -24, 1.5 * 2.0 ** -24, 2.0 ** -24, 6.1e-5, 3e-6, -3e-6,
           2.0 ** -25 * (1 + 2.0 ** -20)]
    flush = [2.0 ** -25, -2.0 ** -25, 2.0 ** -26, 1e-10, -1e-30, 1e-45, 0.0, -0.0]
    top = [65504.0, 65519.99, 65520.0, -65519.99, -65520.0, 65536.0, 1e9, 3.4e38, np.inf, -np.inf, np.nan]
    return np.array(ties + sub + flush + top, dtype=np.float32)


def _guarded(body, dtype):
    """``body`` [rows, pitch] in front of GUARD sentinels, flat."""
    return np.concatenate([body.astype(dtype).ravel(), np.full(GUARD, SENTINEL, dtype=dtype)])


@functools.lru_cache(maxsize=None)
def cvt_case(shape):
    """dict src32 / want16 (npm_cvt_f32_f16) and src16 / want32 (npm_cvt_f16_f32), whole guarded buffers.  The values: N(0, 1),
    the special set at the front and once more at the very end, where every looping cap is past its first trip."""
    cols, p32, p16 = shape
    rng = np.random.default_rng(cols)
    special = special_floats()
    data = rng.standard_normal(CVT_ROWS * cols).astype(np.float32)
    data[:special.size] = special
    data[-special.size:] = special
    data = data.reshape(CVT_ROWS, cols)
    with np.errstate(over='ignore'):
        halves = data.astype(np.float16)
    src32, want32 = (np.full([CVT_ROWS, p32], SENTINEL, dtype=np.float32) for _ in range(2))
    src16, want16 = (np.full([CVT_ROWS, p16], SENTINEL, dtype=np.float16) for _ in range(2))
    src32[:, :cols], want16[:, :cols] = data, halves
    src16[:, :cols], want32[:, :cols] = halves, halves.astype(np.float32)
    return dict(src32=_guarded(src32, np.float32), want16=_guarded(want16, np.float16), src16=_guarded(src16, np.float16),
                want32=_guarded(want32, np.float32), first_special=CVT_ROWS * cols - special.size)


@functools.lru_cache(maxsize=None)
def take_case(shape):
    """dict src [11, pitch] flat, idx, want (the guarded destination): dst[r, :cols] = src[idx[r], :cols], zeros for -1 and 11."""
    cols, sp, dp = shape
    rng = np.random.default_rng(cols)
    src = rng.standard_normal([TAKE_SRC_ROWS, sp]).astype(np.float32)
    want = np.full([TAKE_ROWS, dp], SENTINEL, dtype=np.float32)
    for r, from_ in enumerate(TAKE_IDX):
        want[r, :cols] = src[from_, :cols] if 0 <= from_ < TAKE_SRC_ROWS else 0.0
    return dict(src=src.ravel(), idx=np.array(TAKE_IDX, dtype=np.int32), want=_guarded(want, np.float32))


def take_rows_outside_in_tail(shape, cap):
    """Destination rows of zeros (an index outside the source) that have an item in a trip >= 2."""
    per_row = take_per_row(*shape)
    lanes = ew_lanes(TAKE_ROWS * per_row, cap)
    return [r for r, from_ in enumerate(TAKE_IDX) if not 0 <= from_ < TAKE_SRC_ROWS and (r + 1) * per_row > lanes]


# ---- b. the row copies ------------------------------------------------------------------------------------------------------------------
ROW_LEN, ROW_B = 1024, 71
ROW_T = {'f32': 30, 'f16': 60}                      # new tokens of an append, rows of a gather: 71 x 30 x 256 = 71 x 60 x 128 = 545 280
ROW_CACHE_ROWS = {'f32': 48, 'f16': 80}             # rows per sequence: 3 / 5 pages
ROW_PAGE, ROW_SPARE_PAGES = 16, 5
ROW_CACHE_PITCH = ROW_LEN + 8                       # elements of the cache's type
ROW_AT = 7                                          # the uniform append
ROW_SOURCES = {'pitched': (ROW_LEN + 8, 0), 'packed': (ROW_LEN + 64, 32)}     # (pitch, offset of the row inside it), floats
ROW_DTYPE = {'f32': np.float32, 'f16': np.float16}
ROW_OUTSIDE_PAGE = -1                               # table entries that no gather may read (tests/test_gpu_kv16.py)
APPEND_CASES = tuple(itertools.product(('f32', 'f16'), ('uniform', 'varlen', 'paged'), ('pitched', 'packed')))
GATHER_CASES = tuple(itertools.product(('f32', 'f16'), ('varlen', 'paged')))


def row_total(kv):
    """row_copy: ``total = (long)batch * count * (row_len / W)``."""
    return ROW_B * ROW_T[kv] * (ROW_LEN // ROW_W[kv])


def row_lens(kv):
    """new_lens of an append / lens of a gather.  Trip 2 is the end of sequence 68 and all of 69 and 70: full, 0, partial, with a
    full one (67) next to them.  Sequences 0 .. 2 are what the lanes of trip 2 see on trip 1: 5, 10 and 0 rows, so that lanes that
    skip there store behind it.  The others are random in 0 .. T."""
    t = ROW_T[kv]
    n = np.random.default_rng(t).integers(0, t + 1, ROW_B)
    n[:3] = (5, 10, 0)
    n[67:] = (t, t, 0, t // 2 - 2)
    return n.astype(np.int32)


def row_at_lens(kv):
    return np.random.default_rng(ROW_T[kv] + 1).integers(0, ROW_CACHE_ROWS[kv] - ROW_T[kv] + 1, ROW_B).astype(np.int32)


def row_facts(kv, ragged=True):
    """kv_append_kernel / kv_gather_kernel's decode of every item, as ``rope_facts``: a row t >= lens[b] is one the append skips and
    the gather zeroes."""
    per_row, t_ = ROW_LEN // ROW_W[kv], ROW_T[kv]
    total = row_total(kv)
    lanes = row_copy_lanes(total)
    i = np.arange(total)
    row = i // per_row
    b, t = row // t_, row % t_
    skipped = t >= row_lens(kv)[b] if ragged else np.zeros(total, dtype=bool)
    tail = i >= lanes
    tail_b = sorted(set(b[tail].tolist()))
    return dict(total=total, lanes=lanes, trips=trips(total, lanes), partial=total % lanes != 0, skipped=bool((skipped & tail).any()),
                stored=bool((~skipped & tail).any()), sequences=tail_b, resumes=_resumes(skipped, lanes),
                tail_lens=[int(row_lens(kv)[s]) for s in tail_b], first_tail_row=(int(b[tail][0]), int(t[tail][0])))


@functools.lru_cache(maxsize=None)
def row_source(kv, source):
    """The fp32 rows of an append, [B T, pitch] flat: N(0, 1) everywhere, so a column decoded wrongly brings a different value."""
    pitch, _ = ROW_SOURCES[source]
    return np.random.default_rng(ROW_T[kv] + pitch).standard_normal(ROW_B * ROW_T[kv] * pitch).astype(np.float32)


@functools.lru_cache(maxsize=None)
def row_tables(kv):
    """(block table [B, pages per sequence], pages in the pool): a shuffled assignment, ROW_SPARE_PAGES pages that nobody owns."""
    per_seq = ROW_CACHE_ROWS[kv] // ROW_PAGE
    pages = ROW_B * per_seq + ROW_SPARE_PAGES
    order = np.random.default_rng(per_seq).permutation(pages)
    return order[:ROW_B * per_seq].reshape(ROW_B, per_seq).astype(np.int32), pages


def _cache_rows(flat, kv, layout):
    """[B, cache rows, pitch] view of a flat cache buffer; a paged one through the block table (a copy, with the index to put it back)."""
    rows, pitch = ROW_CACHE_ROWS[kv], ROW_CACHE_PITCH
    if layout != 'paged':
        return flat[:ROW_B * rows * pitch].reshape(ROW_B, rows, pitch), None
    table, pages = row_tables(kv)
    pool = flat[:pages * ROW_PAGE * pitch].reshape(pages, ROW_PAGE, pitch)
    return pool, table


def row_cache_elems(kv, layout):
    pages = row_tables(kv)[1] if layout == 'paged' else ROW_B * ROW_CACHE_ROWS[kv] // ROW_PAGE
    return pages * ROW_PAGE * ROW_CACHE_PITCH


def append_case(kv, layout, source):
    """dict src (flat fp32), offset, pitch, cache0 / want (the guarded cache before and after), at, at_lens, new_lens, table, and
    the geometry.  Row at_b + t of sequence b = src[b T + t, offset : offset + 1024] for t < new_lens[b] (every t in the uniform
    append), rounded by ``astype`` for an fp16 cache; every other element of the cache keeps its sentinel."""
    t_, dtype = ROW_T[kv], ROW_DTYPE[kv]
    pitch, offset = ROW_SOURCES[source]
    src = row_source(kv, source)
    n = row_lens(kv) if layout != 'uniform' else np.full(ROW_B, t_, dtype=np.int32)
    at = row_at_lens(kv) if layout != 'uniform' else np.full(ROW_B, ROW_AT, dtype=np.int32)
    elems = row_cache_elems(kv, layout)
    cache0 = np.full(elems + GUARD, SENTINEL, dtype=dtype)
    want = cache0.copy()
    b, t = np.nonzero(np.arange(t_)[None, :] < n[:, None])
    rows = src.reshape(ROW_B * t_, pitch)[b * t_ + t, offset:offset + ROW_LEN].astype(dtype)
    view, table = _cache_rows(want, kv, layout)
    j = at[b] + t
    if table is None:
        view[b, j, :ROW_LEN] = rows
    else:
        view[table[b, j // ROW_PAGE], j % ROW_PAGE, :ROW_LEN] = rows
    return dict(src=src, pitch=pitch, offset=offset, cache0=cache0, want=want, at_lens=at, new_lens=n,
                table=row_tables(kv)[0] if layout == 'paged' else None, stored_rows=int(b.size),
                stride=ROW_PAGE * ROW_CACHE_PITCH if layout == 'paged' else ROW_CACHE_ROWS[kv] * ROW_CACHE_PITCH)


def gather_case(kv, layout):
    """dict cache (flat, every row and the padding random), lens, table (entries behind a sequence's last page: ROW_OUTSIDE_PAGE),
    out0 / want (the guarded [B, T, 1024] destination): want[b, j] = row j of sequence b for j < lens[b], zeros behind it."""
    t_, dtype = ROW_T[kv], ROW_DTYPE[kv]
    lens = row_lens(kv)
    elems = row_cache_elems(kv, layout)
    cache = np.random.default_rng(t_ + 2).standard_normal(elems).astype(dtype)
    view, table = _cache_rows(cache, kv, layout)
    out0 = np.full(ROW_B * t_ * ROW_LEN + GUARD, SENTINEL, dtype=np.float32)
    want = out0.copy()
    body = want[:ROW_B * t_ * ROW_LEN].reshape(ROW_B, t_, ROW_LEN)
    body[:] = 0.0
    b, j = np.nonzero(np.arange(t_)[None, :] < lens[:, None])
    if table is None:
        body[b, j] = view[b, j, :ROW_LEN].astype(np.float32)
    else:
        body[b, j] = view[table[b, j // ROW_PAGE], j % ROW_PAGE, :ROW_LEN].astype(np.float32)
        table = table.copy()
        for s in range(ROW_B):
            table[s, -(-int(lens[s]) // ROW_PAGE):] = ROW_OUTSIDE_PAGE
    return dict(cache=cache, lens=lens, table=table, out0=out0, want=want,
                stride=ROW_PAGE * ROW_CACHE_PITCH if layout == 'paged' else ROW_CACHE_ROWS[kv] * ROW_CACHE_PITCH)


# ---- c. the page copies -----------------------------------------------------------------------------------------------------------------
PageCase = namedtuple('PageCase', 'name page_bytes row_bytes pages n planes plane_bytes dtype')
PIECE_ROWS, PIECE_ROW_BYTES = 64, 4160              # 266 240 bytes: 16 640 pieces of 16 bytes, 256 of them past 64 x 256 lanes
PIECE_PAIR_ROWS = (64, 63, 1, 0)                    # trip 2 copies for the first pair only; 63 rows end 4 pieces below the lanes
PAIRS = PAGE_COPY_YZ + 5
PLANES = PAGE_COPY_YZ + 3
_PIECE_PAGE = PIECE_ROWS * PIECE_ROW_BYTES
PAGE_CASES = (
    PageCase('pieces-f32', _PIECE_PAGE, PIECE_ROW_BYTES, 9, 4, 2, 10 * _PIECE_PAGE, 'f32'),     # a gap of one page between the planes
    PageCase('pieces-f16', _PIECE_PAGE, PIECE_ROW_BYTES, 9, 4, 2, 10 * _PIECE_PAGE, 'f16'),
    PageCase('pairs-1', 16, 16, 2 * PAIRS + 3, PAIRS, 1, 16 * (2 * PAIRS + 3), 'bytes'),
    PageCase('pairs-3', 16, 16, 2 * PAIRS + 3, PAIRS, 3, 16 * (2 * PAIRS + 4), 'bytes'),        # a gap of one page
    PageCase('planes-32', 16, 16, 2, 1, PLANES, 32, 'bytes'),
    PageCase('planes-48', 16, 16, 2, 1, PLANES, 48, 'bytes'),                                   # a gap of one page
)


def page_trips(c):
    """(pieces, pairs, planes) -> (work, lanes) of the three nested strides; the piece loop of pair i runs to rows[i] * row16."""
    page16 = c.page_bytes // 16
    return dict(pieces=(page16, min(-(-page16 // BLOCK), PAGE_COPY_X) * BLOCK), pairs=(c.n, min(c.n, PAGE_COPY_YZ)),
                planes=(c.planes, min(c.planes, PAGE_COPY_YZ)))


@functools.lru_cache(maxsize=None)
def page_pairs(name):
    """(src pages, dst pages, rows) of a case: all pages distinct, src != dst."""
    c = next(p for p in PAGE_CASES if p.name == name)
    rng = np.random.default_rng(c.n)
    order = rng.permutation(c.pages)
    if name.startswith('pieces'):
        rows = np.array(PIECE_PAIR_ROWS)
    elif name.startswith('pairs'):
        rows = rng.integers(0, 2, c.n)
        rows[-5:] = (1, 0, 1, 1, 0)                                      # both kinds among the pairs of trip 2
    else:
        order, rows = np.array([1, 0]), np.array([1])
    return order[:c.n].astype(np.int32), order[c.n:2 * c.n].astype(np.int32), rows.astype(np.int32)


def _page_view(words, c, planes):
    """[planes, pages, page words] view of a flat uint32 buffer."""
    return np.lib.stride_tricks.as_strided(words, shape=(planes, c.pages, c.page_bytes // 4), strides=(c.plane_bytes, c.page_bytes, 4))


def page_case(name, planes=None):
    """dict pool0 / want as uint32 words (the planes, the gaps and GUARD words behind them) and the pairs.  Source pages hold data
    (floats or halves of the pool's type; random words in the 16-byte cases, where every page does); every other byte of a 'pieces'
    pool holds the sentinel.  ``planes``: fewer than the case has (npm_kv_copy_pages copies the first plane only)."""
    c = next(p for p in PAGE_CASES if p.name == name)
    src, dst, rows = page_pairs(name)
    rng = np.random.default_rng(c.planes)
    words = c.planes * c.plane_bytes // 4
    if c.dtype == 'bytes':
        pool0 = rng.integers(0, 2 ** 32, words + GUARD, dtype=np.uint32)
    else:
        dtype = ROW_DTYPE[c.dtype]
        pool0 = np.full((words + GUARD) * 4 // np.dtype(dtype).itemsize, SENTINEL, dtype=dtype).view(np.uint32)
        data = rng.standard_normal([c.planes, c.n, c.page_bytes // np.dtype(dtype).itemsize]).astype(dtype)
        _page_view(pool0, c, c.planes)[:, src] = data.view(np.uint32)
    want = pool0.copy()
    before, after = _page_view(pool0, c, c.planes), _page_view(want, c, c.planes)
    for r in sorted(set(rows.tolist())):
        which = rows == r
        after[:c.planes if planes is None else planes, dst[which], :r * c.row_bytes // 4] = \
            before[:c.planes if planes is None else planes, src[which], :r * c.row_bytes // 4]
    return dict(case=c, pool0=pool0, want=want, src=src, dst=dst, rows=rows)


# ---- d. the 32-bit index refusal --------------------------------------------------------------------------------------------------------
# batch 2^15, tokens 2^10, D 128 on the vector instance (16 items per head) and 4 heads: 2^15 x 2^10 x 4 x 16 = 2^31 exactly, one
# more than the kernels' index holds.  npm_rope: 4 heads.  npm_rope_kv_append: (H, Hkv) = (2, 1) with tables (4 active heads),
# (2, 2) without (the 4 k and v heads).  at = 0 and a table of exactly ``tokens`` rows pass the checks in front of the refusal.
REFUSE_BATCH, REFUSE_TOKENS, REFUSE_D, REFUSE_HEADS = 1 << 15, 1 << 10, 128, 4
REFUSE_APPEND = (('rope', 2, 1), ('copy', 2, 2))


def refuse_total(active_heads):
    return REFUSE_BATCH * REFUSE_TOKENS * active_heads * rope_pieces(REFUSE_D)
