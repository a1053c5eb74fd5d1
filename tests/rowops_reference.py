"""The row kernels of csrc/npm_rowops.hip, restated: shared by tests/test_rowops_host.py (CPU) and tests/test_gpu_rowops_paths.py.

* ``WIDTHS`` / ``GENERIC_WIDTHS`` / ``ROW_COUNTS``: the width grid.  The launch plan (csrc/npm_row_plan.h) keeps a row in VPL float4 per lane, VPL =
  1 / 2 / 4 / 8 / 16 for rows of <= 256 / 512 / 1024 / 2048 / 4096 floats (``vpl_of``); per class the smallest width (4 floats past
  the class below), a width whose last 64-chunk group is partly filled (where the ``lane + 64 j < nvec`` guards decide) and the
  largest.  Widths that are no multiple of 4 or exceed 4096 take the generic kernels.  Row counts 1 / 5 / 7 / 9: a single row; a
  second and a third block whose last three waves idle; one idle wave in the last block.
* ``softmax_fwd_model`` / ``softmax_bwd_model`` / ``layernorm_fwd_model`` / ``layernorm_bwd_model`` / ``colsum_model``: float32
  NumPy in the kernels' own order -- lane l holds float4 chunks l, l + 64, ...; a lane adds (x + y) + (z + w) per chunk, chunk after
  chunk; the xor butterfly 32 .. 1 joins the lanes.  dgamma / dbeta: a wave sums the rows it owns (row, row + 4 grid, ...), the
  four waves of a block are added in wave order, then a sum in colsum_kernel's manner (16 row lanes, then the lanes in order, row
  chunks of at most 256 blocks) folds the blocks -- in the library's manner, not always with its chunk split (see
  ``layernorm_bwd_model``).  The models do not reproduce hipcc's fused multiply-adds nor the device's expf: they size
  bounds, they do not predict bits.
* ``ln_range`` / ``softmax_range``: the range data.  ``kappa`` and ``cond_fraction``: the conditioned LayerNorm bound,
  tol (|ref| + max |ref|) (1 + kappa / KAPPA_DIV) with kappa = max |x_row| rstd_row in float64: the mean carries about one
  float32 rounding of max |x|, which rstd magnifies in z = (x - mean) rstd.  At the suite's usual 2 N(0, 1) + 0.5 data kappa is
  about 4 and the factor 1.25.
* ``ew_paths`` / ``EW_CAPS`` / ``ew_size``: the loops of the elementwise kernels under a grid cap, recomputed.
* ``ln_walk_rows`` / ``ln_walk_counts``: the shape that gives some waves of the LayerNorm backward three rows and the others two.
"""

import numpy as np

F = np.float32
WAVE = 64
ROWS_PER_BLOCK = 4
VPLS = (1, 2, 4, 8, 16)
WIDTHS = ((4, 72, 256), (260, 388, 512), (516, 900, 1024), (1028, 1540, 2048), (2052, 3076, 4096))   # per VPL: smallest, partly filled, largest
GENERIC_WIDTHS = (33, 1001, 4100, 5000)
ALL_WIDTHS = tuple(w for ws in WIDTHS for w in ws) + GENERIC_WIDTHS
ROW_COUNTS = (1, 5, 7, 9)
ONE_PER_CLASS = (72, 388, 900, 2048, 3076)        # dropout forms and range data: one width per VPL
WALK_WIDTHS = (72, 260, 900, 2048, 3076)          # the backward's row walk
NT_WIDTHS = (256, 512, 1024, 2048, 4096)          # >= 32 MB
NT_BYTES = 1 << 25                                # stream_nt(): tensors of at least this many bytes take the NT instances
NT_ELEMS = 1 << 23
CUS = 256                                         # MI355X; the GPU tests read the device's figure
LN_BWD_BLOCKS_PER_CU = 4
EPS = 1e-3
KAPPA_DIV = 8.0
TOL_Z, TOL_STAT, TOL_DX, TOL_SOFTMAX, TOL_SOFTMAX_BWD, TOL_SAME, TOL_COLSUM, TOL_ROWDOT = 3e-6, 2e-6, 5e-6, 2e-6, 5e-6, 5e-7, 2e-6, 3e-6


def vpl_of(n):
    """Float4 per lane of the row-in-registers kernels, None for the generic ones."""
    if n % 4 or n > 4096 or n < 4:
        return None
    return next(v for v in VPLS if n <= 256 * v)


def chunk_groups(n):
    """(full 64-chunk groups, chunks in the last partly filled group)."""
    return (n // 4) // WAVE, (n // 4) % WAVE


def nt_rows(d):
    return NT_ELEMS // d + 3


# ---- the kernels' order in float32 ------------------------------------------------------------------------------------------
def _lanes(x, vpl, fill=0.0):
    """[rows, n] -> [rows, vpl, 64, 4]: chunk lane + 64 j sits at [:, j, lane]."""
    rows, n = x.shape
    buf = np.full((rows, vpl * 256), fill, dtype=F)
    buf[:, :n] = x
    return buf.reshape(rows, vpl, WAVE, 4)


def _lane_sum(t):
    s = np.zeros((t.shape[0], WAVE), dtype=F)
    for j in range(t.shape[1]):
        s = s + ((t[:, j, :, 0] + t[:, j, :, 1]) + (t[:, j, :, 2] + t[:, j, :, 3]))
    return s


def _lane_sum_generic(x):
    """Lane l adds elements l, l + 64, ... one by one."""
    rows, n = x.shape
    steps = -(-n // WAVE)
    buf = np.zeros((rows, steps * WAVE), dtype=F)
    buf[:, :n] = x
    buf = buf.reshape(rows, steps, WAVE)
    s = np.zeros((rows, WAVE), dtype=F)
    for k in range(steps):
        s = s + buf[:, k]
    return s


def _butterfly(v):
    idx = np.arange(WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, idx ^ off]
    return v[:, :1]


def _row_sum(x):
    """wave_sum of the per-lane sums of a [rows, n] float32 tensor -> [rows, 1]."""
    x = np.ascontiguousarray(x, dtype=F)
    vpl = vpl_of(x.shape[1])
    return _butterfly(_lane_sum_generic(x) if vpl is None else _lane_sum(_lanes(x, vpl)))


def softmax_fwd_model(x, scale=1.0):
    x = np.asarray(x, dtype=F)
    with np.errstate(invalid='ignore', over='ignore'):
        v = x * F(scale)
        e = np.exp(v - v.max(axis=1, keepdims=True)).astype(F)
        return e * (F(1) / _row_sum(e))


def softmax_bwd_model(y, dy, scale=1.0):
    y, dy = np.asarray(y, dtype=F), np.asarray(dy, dtype=F)
    with np.errstate(invalid='ignore'):
        dot = _row_sum(y * dy)
        return F(scale) * y * (dy - dot)


def layernorm_fwd_model(x, gamma, beta, eps=EPS):
    """Returns (z, mean [rows], rstd [rows])."""
    x, gamma, beta = np.asarray(x, dtype=F), np.asarray(gamma, dtype=F), np.asarray(beta, dtype=F)
    d = x.shape[1]
    mean = _row_sum(x) / F(d)
    c = x - mean                                            # padding never enters: the kernel's chunk guard
    var = _row_sum(c * c) / F(d)
    rstd = F(1) / np.sqrt(var + F(eps), dtype=F)
    return gamma * (c * rstd) + beta, mean[:, 0], rstd[:, 0]


def colsum_strip_plan(rows, cols):
    """colsum_run's split for the strip kernel: (strips of 64 columns, row chunks, rows per chunk, rows of the last chunk)."""
    strips = -(-cols // 64)
    chunks = max(1, min(-(-rows // 256), max(1, 2048 // strips)))
    rpc = -(-rows // chunks)
    chunks = -(-rows // rpc)
    return strips, chunks, rpc, rows - (chunks - 1) * rpc


def colsum_strip_trips(rows_in_chunk):
    """colsum_kernel's vector path over one chunk, for every row lane: (set of trip counts of the four-row unrolled body, set of
    trip counts of the single-row remainder)."""
    unrolled, rest = set(), set()
    for rl in range(16):
        r, u = rl, 0
        while r + 48 < rows_in_chunk:
            r, u = r + 64, u + 1
        unrolled.add(u)
        rest.add(len(range(r, rows_in_chunk, 16)))
    return unrolled, rest


def colsum_model(x):
    """colsum_kernel: 16 row lanes add rows rl, rl + 16, ... in order, the lanes are added in order; more than 256 rows are cut
    into chunks whose partial sums go through the same kernel once more."""
    x = np.asarray(x, dtype=F)
    rows, cols = x.shape

    def one(block):
        r = block.shape[0]
        steps = -(-r // 16)
        buf = np.zeros((steps * 16, cols), dtype=F)
        buf[:r] = block
        buf = buf.reshape(steps, 16, cols)
        acc = np.zeros((16, cols), dtype=F)
        for k in range(steps):
            acc = acc + buf[k]
        s = np.zeros(cols, dtype=F)
        for i in range(16):
            s = s + acc[i]
        return s

    _, chunks, rpc, _ = colsum_strip_plan(rows, cols)
    if chunks <= 1:
        return one(x)
    return one(np.stack([one(x[c * rpc:(c + 1) * rpc]) for c in range(chunks)]))


def ln_bwd_grid(rows, blocks_per_cu=LN_BWD_BLOCKS_PER_CU, cus=CUS):
    return min(-(-rows // ROWS_PER_BLOCK), blocks_per_cu * cus)


def layernorm_bwd_model(dz, x, mean, rstd, gamma, residual=None, grid=None):
    """Returns (dx, dgamma, dbeta) from the forward's float32 mean / rstd, as the kernel takes them.  The block partials are folded
    by ``colsum_model`` on a [grid, d] array; the library folds [grid, 2 d] (or d columns at a pitch of 2 d), whose split into row
    chunks can differ from this one where 2 d has more strips: the same kind of sum, not always the same grouping."""
    dz, x, gamma = np.asarray(dz, dtype=F), np.asarray(x, dtype=F), np.asarray(gamma, dtype=F)
    rows, d = x.shape
    mu, rs = np.asarray(mean, dtype=F).reshape(rows, 1), np.asarray(rstd, dtype=F).reshape(rows, 1)
    yh = (x - mu) * rs
    g = dz * gamma
    if vpl_of(d) is None:
        m1, m2 = _row_sum(g) / F(d), _row_sum(g * yh) / F(d)
    else:
        inv_d = F(1) / F(d)
        m1, m2 = _row_sum(g) * inv_d, _row_sum(g * yh) * inv_d
    dx = rs * ((g - m1) - yh * m2)
    if residual is not None:
        dx = dx + np.asarray(residual, dtype=F)
    if vpl_of(d) is None:
        return dx, colsum_model(dz * yh), colsum_model(dz)
    grid = ln_bwd_grid(rows) if grid is None else grid
    waves = ROWS_PER_BLOCK * grid
    steps = -(-rows // waves)

    def fold(t):
        buf = np.zeros((steps * waves, d), dtype=F)
        buf[:rows] = t
        buf = buf.reshape(steps, waves, d)
        acc = np.zeros((waves, d), dtype=F)
        for k in range(steps):                          # a wave's own rows, in order
            acc = acc + buf[k]
        acc = acc.reshape(grid, ROWS_PER_BLOCK, d)
        return colsum_model(((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3])

    return dx, fold(dz * yh), fold(dz)


# ---- fp64 references and bounds -----------------------------------------------------------------------------------------------
def fraction(got, ref, tol, scale=None):
    """Largest fraction of conftest.assert_close's bound tol (|ref| + max |ref|) that ``got`` uses; inf for a non-finite
    difference where the reference is finite."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not ref.size:
        return 0.0
    scale = np.abs(ref).max() if scale is None else scale
    err = np.abs(got - ref) / (tol * (np.abs(ref) + scale) + 1e-30)
    return float(np.where(np.isnan(err), np.inf, err).max())


def kappa(x, eps=EPS):
    """max |x_row| rstd_row in float64, [rows]."""
    x = np.asarray(x, dtype=np.float64)
    return np.abs(x).max(axis=1) / np.sqrt(x.var(axis=1) + eps)


def cond_fraction(got, ref, tol, k, scale=None):
    """``fraction`` under the conditioned bound: row r may use (1 + k[r] / KAPPA_DIV) times the plain bound."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = np.abs(ref).max() if scale is None else scale
    widen = (1.0 + np.asarray(k, dtype=np.float64) / KAPPA_DIV).reshape([-1] + [1] * (ref.ndim - 1))
    err = np.abs(got - ref) / ((tol * (np.abs(ref) + scale) + 1e-30) * widen)
    return float(np.where(np.isnan(err), np.inf, err).max())


def layernorm_ref(x, gamma, beta, dz, residual=None, eps=EPS):
    """float64 on the float32 inputs: dict z, mean, rstd, dx, dgamma, dbeta."""
    x, gamma, beta, dz = (np.asarray(a, dtype=np.float64) for a in (x, gamma, beta, dz))
    mean = x.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(x.var(axis=1, keepdims=True) + eps)
    yh = (x - mean) * rstd
    g = dz * gamma
    dx = rstd * (g - g.mean(axis=1, keepdims=True) - yh * (g * yh).mean(axis=1, keepdims=True))
    if residual is not None:
        dx = dx + np.asarray(residual, dtype=np.float64)
    return dict(z=gamma * yh + beta, mean=mean[:, 0], rstd=rstd[:, 0], dx=dx, dgamma=(dz * yh).sum(axis=0), dbeta=dz.sum(axis=0))


def ln_range_fractions(kind, x, gamma, beta, dz, got):
    """Fractions of the conditioned bound of ``got`` (z, mean, rstd, dx, dgamma) on one kind of range rows.  Constant rows: z,
    mean and rstd only -- the exact yhat is 0 there, so dgamma and the yhat term of dx have no scale to be relative to; dx must
    be finite."""
    ref = layernorm_ref(x, gamma, beta, dz)
    k = kappa(x)
    fr = dict(z=cond_fraction(got['z'], ref['z'], TOL_Z, k),
              mean=cond_fraction(got['mean'], ref['mean'], TOL_STAT, k, scale=float(np.abs(x).max())),
              rstd=cond_fraction(got['rstd'], ref['rstd'], TOL_STAT, k))
    if kind != 'constant':
        fr.update(dx=cond_fraction(got['dx'], ref['dx'], TOL_DX, k),
                  dgamma=cond_fraction(got['dgamma'], ref['dgamma'], TOL_DX, np.full(1, k.max())))
    return fr


def softmax_ref(x, scale=1.0):
    with np.errstate(invalid='ignore'):
        v = np.float64(scale) * np.asarray(x, dtype=np.float64)
        e = np.exp(v - v.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)


def softmax_bwd_ref(y, dy, scale=1.0):
    y, dy = np.asarray(y, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return scale * y * (dy - (y * dy).sum(axis=1, keepdims=True))


# ---- data ---------------------------------------------------------------------------------------------------------------------
def grid_data(rows, d, seed=0):
    """The suite's usual LayerNorm data (2 N(0, 1) + 0.5) and N(0, 1) parameters and gradients."""
    rng = np.random.default_rng(1000 * seed + 7 * rows + d)
    return dict(x=(rng.standard_normal((rows, d)) * 2 + 0.5).astype(F), gamma=rng.standard_normal(d).astype(F),
                beta=rng.standard_normal(d).astype(F), dz=rng.standard_normal((rows, d)).astype(F),
                res=rng.standard_normal((rows, d)).astype(F))


def softmax_data(rows, n, seed=0):
    rng = np.random.default_rng(1000 * seed + 31 * rows + n)
    return (rng.standard_normal((rows, n)) * 4).astype(F), rng.standard_normal((rows, n)).astype(F)


LN_SHIFTS = ((100.0, 1.0), (1e3, 1.0), (1e4, 1.0), (1e3, 0.05), (-3e4, 10.0))
LN_RANGE_KINDS = tuple('shift_%g_%g' % s for s in LN_SHIFTS) + ('constant', 'outlier', 'tiny')


def ln_range(kind, d, seed=0):
    """[3, d] float32 rows of one kind."""
    rng = np.random.default_rng(100 * seed + d + 13 * LN_RANGE_KINDS.index(kind))
    base = rng.standard_normal((3, d))
    if kind.startswith('shift_'):
        shift, std = LN_SHIFTS[LN_RANGE_KINDS.index(kind)]
        x = shift + std * base
    elif kind == 'constant':                               # variance 0: rstd = 1 / sqrt(eps)
        x = np.repeat(np.array([[0.1], [7.0], [-2.7]]), d, axis=1)
    elif kind == 'outlier':
        x = base
        for r, at in enumerate((0, d // 2, d - 1)):
            x[r, at] = 1e6
    else:                                                  # variance far below eps
        x = 1e-20 * base
    return x.astype(F)


def softmax_range(n, seed=0):
    """(x [9, n] float32, index of the row that is -inf throughout).  Rows 0 / 1 shifted by +-1e4, 2 / 3 spanning 200 units,
    4 -inf at scattered positions, 5 a whole leading 64-chunk group (256 floats, or half the row where that is all of it) -inf,
    6 the tail -inf, 7 both and scattered ones, 8 all -inf."""
    rng = np.random.default_rng(100 * seed + n)
    x = rng.standard_normal((9, n)) * 4
    x[0] += 1e4
    x[1] -= 1e4
    x[2] = rng.uniform(-100, 100, n)
    x[3] = rng.uniform(-100, 100, n)
    x[2, 0], x[2, n - 1], x[3, n // 2], x[3, n // 3] = 100, -100, 100, -100
    lead = 256 if n > 256 else n // 2
    tail = n - max(1, n // 3)
    scattered = rng.random(n) < 0.3
    scattered[n // 2] = False
    x[4, scattered] = -np.inf
    x[5, :lead] = -np.inf
    x[6, tail:] = -np.inf
    x[7, :lead] = -np.inf
    x[7, tail:] = -np.inf
    x[7, scattered] = -np.inf
    if np.isinf(x[7]).all():
        x[7, n // 2] = 0.5
    x[8] = -np.inf
    return x.astype(F), 8


# ---- the elementwise kernels under a grid cap ------------------------------------------------------------------------------------
EW_CAPS = (1, 2, 3)
EW_UNROLL = 4
EW_BLOCK = 256


def ew_size(cap):
    """n = 4 (one full unrolled trip + a remainder of one stride and 37 chunks) + 3."""
    stride = cap * EW_BLOCK
    return 4 * (EW_UNROLL * stride + stride + 37) + 3


def ew_paths(n, cap):
    """ew1_kernel / ew2_kernel's loops recomputed for every thread: dict grid, unrolled (threads that run the unrolled body),
    unrolled_trips (most trips of one thread), remainder (the set of per-thread trip counts of the remainder loop), tail
    (elements the scalar tail writes), covered (every float4 chunk written exactly once)."""
    nv = n // 4
    grid = max(1, min(-(-(nv + 1) // EW_BLOCK), cap))
    stride = grid * EW_BLOCK
    seen = np.zeros(nv, dtype=np.int64)
    unrolled, most, rem = 0, 0, set()
    for t in range(stride):
        i, trips = t, 0
        while i + (EW_UNROLL - 1) * stride < nv:
            for u in range(EW_UNROLL):
                seen[i + u * stride] += 1
            i += EW_UNROLL * stride
            trips += 1
        unrolled += trips > 0
        most = max(most, trips)
        k = 0
        while i < nv:
            seen[i] += 1
            i += stride
            k += 1
        rem.add(k)
    tail = sum(1 for t in range(stride) if 4 * nv + t < n)
    return dict(grid=grid, stride=stride, unrolled=unrolled, unrolled_trips=most, remainder=rem, tail=tail, covered=bool((seen == 1).all()))


# ---- the LayerNorm backward's row walk ---------------------------------------------------------------------------------------------
def ln_walk_rows(cus=CUS):
    """With one block per CU (NPM_TUNE_LN_BWD_BLOCKS = 1): 4 CUs waves; 2 (4 CUs) + (4 CUs) / 2 + 3 rows."""
    return 2 * 4 * cus + 4 * cus // 2 + 3


def ln_walk_counts(rows, grid):
    """How many waves own 0, 1, 2, ... rows: {rows owned: waves}."""
    waves = ROWS_PER_BLOCK * grid
    owned = [len(range(w, rows, waves)) for w in range(waves)]
    return {k: owned.count(k) for k in sorted(set(owned))}


# ---- column sums of at least 32 MB --------------------------------------------------------------------------------------------------
# 128 divides 1024: the whole-line kernel.  130: the strip kernel's scalar branch (a pitch that is no multiple of 4).  132 and 200:
# its float4 branch (multiples of 4 that do not divide 1024), where the NT instances' loads and stores are.
COLSUM_EDGE_ROWS = (63, 64, 65, 127, 128, 129, 510, 512, 577)    # rows per chunk 63 .. 129 (one chunk), 255, 256 (two), 193 (three)
COLSUM_NT_COLS = (128, 130, 132, 200)


def colsum_nt_rows(cols):
    """Rows of the >= 32 MB column-sum case: a multiple of 8 for the whole-line kernel, 2^23 / cols + 3 for the strip kernel."""
    return (NT_ELEMS // cols + 8) // 8 * 8 if 1024 % cols == 0 else NT_ELEMS // cols + 3


# ---- the whole-line column sum ----------------------------------------------------------------------------------------------------
COLSUM_BLOCKS_PER_CU = 8


def colsum_lines_plan(lines, cus=CUS):
    """colsum_run's split of ``lines`` 4 KB lines: (blocks used, lines per block, lines of the last block)."""
    blocks = min(lines // 16, COLSUM_BLOCKS_PER_CU * cus)
    lpb = -(-lines // blocks)
    used = -(-lines // lpb)
    return used, lpb, lines - (used - 1) * lpb


def colsum_line_cases(cus=CUS, least=4096):
    """{n % 8: lines} for n % 8 in 0, 3, 4, 7, n >= 4 the line count of the last block: the four exits of colsum_lines_kernel's
    pipeline (the closing pair, the closing pair and a tail of three single lines, one closing group, one group and the tail).
    ``least`` 4096 lines are 2^22 elements, where colsum_run starts to take this kernel."""
    found, lines = {}, least
    while len(found) < 4:
        last = colsum_lines_plan(lines, cus)[2]
        if last >= 4 and last % 8 in (0, 3, 4, 7):
            found.setdefault(last % 8, lines)
        lines += 1
    return found
