"""TEST INFRASTRUCTURE ONLY -- the fixed case lists of the GEMM epilogue tests, the harness that launches them through
``device.gemm`` and the references they are held to.  tests/test_gemm_epilogue_host.py proves on the CPU (tests/hostsim/) that
every case meets the LDS-DMA predicate of ``npm_sgemm``, that every family reaches the ``write_tile_buf`` instance its name says,
and that harness and references are right; tests/test_gpu_gemm_epilogue.py then runs the same lists on the device.

A *family* is (epilogue flags, alpha == 1 or not, column sums requested or not): one per branch of ``write_tile_buf`` /
``rmw_epilogue<F, CS>`` (csrc/npm_mfma_tile.h).  The row-dot form is not a family here: it admits one layout and N % 128 == 0
only and has ``test_rowdot_epilogue`` of tests/test_gpu_gemm.py.

Storage of every case: operand pitches are multiples of 4 floats (the DMA kernel needs 16-byte rows) with NaN in the padding
columns; C, the residual and ``aux`` have pairwise different pitches (n + 4, n + 1, n + 3; batched: 3 (n + 4) and 1 resp. 3 less),
each inside an allocation whose guard words and padding columns hold a sentinel NaN that must survive the launch bit for bit;
bias, ``rowvec`` and ``colsum`` sit between guard words too.  A residual that aliases C necessarily shares its pitch.
"""

from __future__ import annotations

import itertools
from typing import NamedTuple, Optional, Tuple

import numpy as np

from conftest import assert_close

BIAS, RESIDUAL, RELU_SAVE, RELU_MASK, RELU, SOFTMAX_BWD = 1, 2, 4, 8, 16, 32        # include/npm_hip.h NPM_EPI_*
ONE = 64                                                                            # rmw_epilogue's "alpha is 1" bit
TUNE_PIPELINE, TUNE_GROUP_M, TUNE_BUF_EPILOGUE, TUNE_WIDE_TILE = 0, 2, 3, 5          # include/npm_hip.h NPM_TUNE_GEMM_*
BM = BN = 128
GK = 16

LAYOUTS = ['NN', 'NT', 'TN']


class Family(NamedTuple):
    name: str
    flags: int
    alpha: float
    colsum: bool
    alias: bool               # the residual IS C (accumulate in place)
    instance: tuple           # the branch of write_tile_buf this family is named after (see ``instance_of``)


def _f(name, flags, alpha, instance, colsum=False, alias=False):
    return Family(name, flags, alpha, colsum, alias, instance)


FAMILIES = [
    # store-only (npm_mfma_tile.h:354-392)
    _f('plain', 0, 1.0, ('store', 'a')),
    _f('plain_half', 0, 0.5, ('store', 'alpha*a')),
    _f('bias', BIAS, 1.0, ('store', 'a+bias')),
    _f('bias_neg2', BIAS, -2.0, ('store', 'generic', False)),
    # read-modify-write, specialised at compile time (npm_mfma_tile.h:403-410)
    _f('bias_res', BIAS | RESIDUAL, 1.0, ('rmw', BIAS | RESIDUAL | ONE, False)),
    _f('res', RESIDUAL, 1.0, ('rmw', RESIDUAL | ONE, False)),
    _f('res_alias', RESIDUAL, 1.0, ('rmw', RESIDUAL | ONE, False), alias=True),
    _f('bias_relu_save', BIAS | RELU_SAVE, 1.0, ('rmw', BIAS | RELU_SAVE | ONE, False)),
    _f('relu_save', RELU_SAVE, 1.0, ('rmw', RELU_SAVE | ONE, False)),
    _f('relu_mask', RELU_MASK, 1.0, ('rmw', RELU_MASK | ONE, False)),
    _f('relu_mask_res', RELU_MASK | RESIDUAL, 1.0, ('rmw', RELU_MASK | RESIDUAL | ONE, False)),
    _f('softmax_bwd', SOFTMAX_BWD, 1.0, ('rmw', SOFTMAX_BWD, False)),
    _f('softmax_bwd_eighth', SOFTMAX_BWD, 0.125, ('rmw', SOFTMAX_BWD, False)),
    # the run-time instance (npm_mfma_tile.h:411)
    _f('bias_res_half', BIAS | RESIDUAL, 0.5, ('rmw', -1, False)),
    _f('relu_mask_res_neg2', RELU_MASK | RESIDUAL, -2.0, ('rmw', -1, False)),
    _f('bias_relu_mask', BIAS | RELU_MASK, 1.0, ('rmw', -1, False)),
    _f('bias_res_relu_save', BIAS | RESIDUAL | RELU_SAVE, 1.0, ('rmw', -1, False)),
    # column sums of the stored C in the epilogue
    _f('relu_mask_colsum', RELU_MASK, 1.0, ('rmw', RELU_MASK | ONE, True), colsum=True),
    _f('plain_colsum', 0, 1.0, ('store', 'generic', True), colsum=True),
    _f('bias_res_colsum', BIAS | RESIDUAL, 1.0, ('rmw', -1, True), colsum=True),
]
FAMILY = {f.name: f for f in FAMILIES}
# The layers take their bias gradients elsewhere today (mlp.py: npm_relu_bwd_colsum), so no layout is "the one the layers use":
# the column-sum families run in all three, like every other family.
COLSUM_LAYOUTS = LAYOUTS


def instance_of(flags: int, alpha: float, colsum: bool) -> tuple:
    """Which code ``write_tile_buf<WITH_COLSUM>`` runs (csrc/npm_mfma_tile.h:354-411), restated.  ``colsum``: the launch asked
    for column sums, i.e. the WITH_COLSUM instantiation of the kernel with e.cs set (csrc/npm_gemm_plan.h gemm_plan: DMA_COLSUM)."""
    has_bias, relu = bool(flags & BIAS), bool(flags & RELU)
    if not flags & (RESIDUAL | RELU_SAVE | RELU_MASK | SOFTMAX_BWD):                   # :354
        simple = not relu and not colsum                                               # :358
        if simple and not has_bias and alpha == 1.0:                                   # :368
            return ('store', 'a')
        if relu and not has_bias and alpha == 1.0 and not colsum:                      # :370
            return ('store', 'max(a,0)')
        if simple and not has_bias:                                                    # :372
            return ('store', 'alpha*a')
        if simple and alpha == 1.0:                                                    # :374
            return ('store', 'a+bias')
        return ('store', 'generic', colsum)                                            # :376-390
    key = flags | (ONE if alpha == 1.0 else 0)                                         # :402
    for special, with_cs in ((BIAS | RESIDUAL | ONE, False), (RESIDUAL | ONE, False), (BIAS | RELU_SAVE | ONE, False),
                             (RELU_SAVE | ONE, False), (RELU_MASK | ONE, True), (RELU_MASK | RESIDUAL | ONE, False)):       # :403-409
        if key == special and (with_cs or not colsum):
            return ('rmw', special, colsum)
    if key & ~ONE == SOFTMAX_BWD and not colsum:                                       # :410
        return ('rmw', SOFTMAX_BWD, False)
    return ('rmw', -1, colsum)                                                         # :411


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------
# Rows: the accumulator rows of a lane sit at (r & 3) + 8 (r >> 2) + 4 half, so 1, 3, 4, 5 end inside the first group of four, 31 / 33
# and 63 / 65 around the MFMA and the wave tile, 97 in the fourth MFMA row, 127 .. 130 around the block tile, 257 a ragged third tile row.
M_CLASSES = [1, 3, 4, 5, 31, 33, 63, 65, 97, 127, 128, 129, 130, 257]
N_CLASSES_NT = [1, 31, 33, 63, 65, 127, 129]                       # B stored [N, K]: any N
MN4_CLASSES = [4, 28, 36, 60, 68, 100, 124, 128, 132, 260]         # an extent that is contiguous in memory: multiples of 4 (float4 rows)
K_CLASSES = [16, 32, 48]                                           # one, two, three K tiles of 16: the loop is unrolled by two stages
BATCH = (2, 3)


def m_classes(layout: str):
    return MN4_CLASSES if layout == 'TN' else M_CLASSES            # A stored [K, M]


def n_classes(layout: str):
    return N_CLASSES_NT if layout == 'NT' else MN4_CLASSES         # B stored [K, N]


class Case(NamedTuple):
    family: str
    layout: str
    m: int
    n: int
    k: int
    batch: Tuple[int, int] = (1, 1)
    split_k: int = 1

    @property
    def what(self):
        return f'{self.family} {self.layout} {self.m}x{self.n}x{self.k} batch={self.batch} split_k={self.split_k}'


def cases(family: str, layout: str):
    """Every M class and every N class of the layout at least once, the pairing shifted from family to family so that the
    families together see more of the product; K cycles through its classes; plus one batched, head-strided case."""
    fi = [f.name for f in FAMILIES].index(family)
    ms, ns = m_classes(layout), n_classes(layout)
    count = max(len(ms), len(ns))
    out = [Case(family, layout, ms[i % len(ms)], ns[(i + fi) % len(ns)], K_CLASSES[(i + fi) % 3]) for i in range(count)]
    out.append(Case(family, layout, 132 if layout == 'TN' else 130, 129 if layout == 'NT' else 132, 32, BATCH))
    return out


GRID = [(f.name, layout) for f in FAMILIES for layout in (COLSUM_LAYOUTS if f.colsum else LAYOUTS)]

# ---- kernels behind knobs ---------------------------------------------------------------------------------------------------------------
WIDE_FAMILIES = ['plain', 'bias_res', 'relu_mask', 'bias_relu_save']
WIDE_LAYOUTS = ['NN', 'NT']


def wide_cases(family: str, layout: str):
    return [Case(family, layout, m, n, 32) for m, n in itertools.product([1, 65, 129, 257], [256, 512])]


PIPELINE_FAMILIES = ['plain', 'bias_res']
PIPELINE_SHAPES = [(128, 128, 32), (256, 384, 96), (64, 16, 32), (128, 128, 0), (130, 132, 48)]      # test_layouts_and_shapes' aligned ones + 1


def pipeline_cases(family: str, layout: str):
    return [Case(family, layout, m, n, k) for m, n, k in PIPELINE_SHAPES]


TILES_M, TILES_N = [1, 7, 8, 9, 17, 19], [1, 2, 3, 5]
GROUP_M = [8, 1, 3]
TILE_MAP_KINDS = {                     # kind -> (tile grids, K, split_k, batch)
    'plain': (list(itertools.product(TILES_M, TILES_N)), 16, 1, (1, 1)),
    'split': ([(1, 1), (7, 2), (8, 3), (9, 5), (17, 1), (19, 2)], 96, 3, (1, 1)),
    'batch': ([(1, 2), (7, 3), (8, 5), (9, 2), (17, 3), (19, 1)], 16, 1, BATCH),
}


def tile_map_cases(kind: str):
    """NN; the last tile row holds one row and the last tile column four columns."""
    grids, k, split, batch = TILE_MAP_KINDS[kind]
    return [Case('plain', 'NN', BM * (tm - 1) + 1, BN * (tn - 1) + 4, k, batch, split) for tm, tn in grids]


# ---- the descriptor and the dispatch of npm_sgemm, restated -------------------------------------------------------------------------------
class Desc(NamedTuple):
    """Everything ``npm_sgemm`` decides on, in elements.  Operands are stored [b0, rows, b1, cols + pad]."""
    lda: int
    ldb: int
    ldc: int
    ldr: int
    ldaux: int
    sa: Tuple[int, int]
    sb: Tuple[int, int]
    sc: Tuple[int, int]
    a_shape: Tuple[int, int]          # (rows, cols) as stored
    b_shape: Tuple[int, int]
    a_pitch: int                      # cols + pad of one head
    b_pitch: int
    c_pitch: int


OPERAND_PAD = 4


def describe(case: Case) -> Desc:
    m, n, k = case.m, case.n, case.k
    b0, b1 = case.batch
    a_shape = (k, m) if case.layout == 'TN' else (m, k)
    b_shape = (n, k) if case.layout == 'NT' else (k, n)
    ap, bp = a_shape[1] + OPERAND_PAD, b_shape[1] + OPERAND_PAD
    cp = n + 4
    ldc = b1 * cp
    fam = FAMILY[case.family]
    if (b0, b1) == (1, 1):
        ldr, ldaux = n + 1, n + 3
    else:
        # the residual and aux are addressed with C's batch strides (csrc/npm_gemm.hip sgemm_glds_kernel): a pitch in [ldc - 4, ldc) keeps the
        # rows of all heads and batches apart
        ldr, ldaux = ldc - 1, ldc - 3
    if fam.alias:
        ldr = ldc
    return Desc(b1 * ap, b1 * bp, ldc, ldr, ldaux, (a_shape[0] * b1 * ap, ap), (b_shape[0] * b1 * bp, bp), (m * ldc, cp),
                a_shape, b_shape, ap, bp, cp)


def takes_dma_kernel(case: Case, pipeline: int = 2, buf_epilogue: int = 1) -> bool:
    """The predicate under which ``npm_sgemm`` launches sgemm_glds_kernel (or the f16x2 kernel, which has the same one) with the
    buffer epilogue: csrc/npm_gemm_plan.h gemm_plan (vec, buf_ok, dma, dma_path) and split_ranges (k_per_split).
    Allocations of the harness are 16-byte aligned (the pool hands out 256-byte aligned blocks, operands start at offset 0)."""
    d, (m, n, k) = describe(case), (case.m, case.n, case.k)
    a_kmaj, b_kmaj = case.layout != 'TN', case.layout == 'NT'
    vec = d.lda % 4 == 0 and d.ldb % 4 == 0 and all(s % 4 == 0 for s in d.sa + d.sb)                       # vec
    vec = vec and (k % 4 == 0 if a_kmaj else m % 4 == 0) and (k % 4 == 0 if b_kmaj else n % 4 == 0)
    fam = FAMILY[case.family]
    fits = lambda ld: (256 * ld + n) * 4 < 2 ** 31
    uses_aux = fam.flags & (RELU_SAVE | RELU_MASK | SOFTMAX_BWD)
    buf_ok = bool(buf_epilogue) and fits(d.ldc) and (not fam.flags & RESIDUAL or fits(d.ldr)) and (not uses_aux or fits(d.ldaux)) and fits(n)
    nkt = (k + 31) // 32                                                                                  # BK = 32
    splits = case.split_k if case.split_k > 1 else 1                                                      # split_k = 1 here
    linear = not fam.flags & (RELU_SAVE | RELU_MASK | RELU | SOFTMAX_BWD)
    if not linear or fam.colsum:
        splits = 1                                                                                        # not linear, or colsum
    splits = max(1, min(splits, nkt))
    per = max(1, -(-nkt // splits))
    k_per_split = per * 32 if splits > 1 else (nkt * 32 if k > 0 else 32)                                 # split_ranges
    tile_n = BN
    a_span = (BM * d.lda + k if a_kmaj else k_per_split * d.lda + BM) * 4                                 # the operand panels
    b_span = (tile_n * d.ldb + k if b_kmaj else k_per_split * d.ldb + tile_n) * 4
    dma = pipeline == 2 and vec and k % GK == 0 and k_per_split % GK == 0 and a_span < 2 ** 31 and b_span < 2 ** 31      # dma
    return dma and buf_ok                                                                                 # dma_path


def takes_wide_tile(case: Case) -> bool:
    """``wide`` of csrc/npm_gemm_plan.h gemm_plan with NPM_TUNE_GEMM_WIDE_TILE = 1, on top of ``takes_dma_kernel``."""
    d = describe(case)
    return takes_dma_kernel(case) and case.n % 256 == 0 and not FAMILY[case.family].colsum and 256 * d.ldb * 4 < 2 ** 30


def expected_math(case: Case, mode: str, wide: bool = False, dma: bool = True) -> str:
    """What ``npm_last_math`` reports after the launch (``math`` of csrc/npm_gemm_plan.h gemm_plan: the table's last column)."""
    if not dma or wide or FAMILY[case.family].colsum:
        return 'f32'
    if mode == 'f16x2' and (case.batch != (1, 1) or case.k == 0):
        return 'bf16x3'
    return mode


def grid_blocks(case: Case) -> int:
    """Blocks of the launch (``grid`` of csrc/npm_gemm_plan.h gemm_plan)."""
    splits = min(case.split_k, (case.k + 31) // 32) if case.split_k > 1 else 1
    return -(-case.m // BM) * -(-case.n // BN) * case.batch[0] * case.batch[1] * splits


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
GUARD = 8
SENTINEL = np.uint32(0x7FC00777).view(np.float32)              # a quiet NaN with a payload: compared bit for bit
SPECIALS = np.array([0.0, -0.0, 1e-30, -1e-30], dtype=np.float32)


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def plant_specials(x: np.ndarray) -> None:
    """+0, -0, 1e-30, -1e-30 at fixed places of every 64 x 64 quadrant of every [m, n] plane of ``x`` ([b0, m, b1, n]), and in
    the last valid row and column; everything else stays as it is (ordinary values)."""
    m, n = x.shape[1], x.shape[3]
    for r0 in range(0, m, 64):
        for c0 in range(0, n, 64):
            h, w = min(64, m - r0), min(64, n - c0)
            for i, v in enumerate(SPECIALS):
                x[:, r0 + (3 * i + 1) % h, :, c0 + (7 * i + 2) % w] = v
                x[:, r0 + (h - 1 - i) % h, :, c0 + (w - 1 - 5 * i) % w] = v
    x[:, m - 1, :, n - 1] = -0.0
    if n > 1:
        x[:, m - 1, :, n - 2] = -1e-30
    if m > 1:
        x[:, m - 2, :, n - 1] = 0.0
    if n > 2:
        x[:, m - 1, :, 0] = 1e-30
    if n > 3:
        x[:, m - 1, :, 1] = 0.0


class Guarded:
    """A host image [GUARD | body | GUARD] of sentinels with a strided [b0, m, b1, n] window into the body."""

    def __init__(self, m, n, batch, ld, s0, s1, extent=None):
        b0, b1 = batch
        need = (b0 - 1) * s0 + (b1 - 1) * s1 + (m - 1) * ld + n
        self.extent = need if extent is None else extent
        assert self.extent >= need
        self.flat = np.full(2 * GUARD + self.extent, SENTINEL, dtype=np.float32)
        self.shape, self.strides = (b0, m, b1, n), (4 * s0, 4 * ld, 4 * s1, 4)
        self.ld = ld
        inside = np.zeros(self.flat.size, dtype=bool)
        self._window(inside.view(np.uint8), 1)[...] = 1
        assert int(inside.sum()) == b0 * m * b1 * n, 'the window overlaps itself'
        self.outside = ~inside

    def _window(self, flat, itemsize=4):
        strides = tuple(s // 4 * itemsize for s in self.strides)
        return np.lib.stride_tricks.as_strided(flat[GUARD:], shape=self.shape, strides=strides)

    def window(self, flat=None):
        return self._window(self.flat if flat is None else flat)

    def upload(self, D):
        self.dev = D.from_host(self.flat)
        return self

    def mat(self, D):
        return D.Mat(self.dev.flat_view(GUARD, [self.extent]), self.ld, self.strides[0] // 4, self.strides[2] // 4)

    def download(self, what):
        """The window's values after a launch; every guard and padding word must still hold the sentinel."""
        flat = self.dev.numpy()
        assert np.array_equal(bits(flat[self.outside]), bits(self.flat[self.outside])), f'{what}: a guard or padding word was written'
        return self.window(flat).copy()

    def unchanged(self, what):
        assert np.array_equal(bits(self.dev.numpy()), bits(self.flat)), f'{what}: an input was written'


def _operand(rng, rows, cols, pitch, batch):
    """[b0, rows, b1, pitch] with NaN behind ``cols``: padding must never reach a stored output."""
    b0, b1 = batch
    x = rng.standard_normal((b0, rows, b1, pitch)).astype(np.float32)
    x[..., cols:] = np.nan
    return x


class Operands:
    """Host data of one case, generated from the case alone, and the operands on the device."""

    def __init__(self, D, case: Case):
        self.D, self.case, self.fam, self.d = D, case, FAMILY[case.family], describe(case)
        fam, d, (m, n, k), batch = self.fam, self.d, (case.m, case.n, case.k), case.batch
        rng = np.random.default_rng([FAMILIES.index(fam), LAYOUTS.index(case.layout), m, n, k, batch[0], case.split_k])
        self.a = _operand(rng, d.a_shape[0], d.a_shape[1], d.a_pitch, batch)
        self.b = _operand(rng, d.b_shape[0], d.b_shape[1], d.b_pitch, batch)
        self.bias = rng.standard_normal(n).astype(np.float32)
        self.zero_row = None
        if fam.flags & RELU_SAVE and not fam.flags & RESIDUAL and m >= 3:
            # the pre-activation itself carries +0 and +-1e-30: a zero row of A times anything is +0, plus these bias values
            self.zero_row = m // 2
            if case.layout == 'TN':
                self.a[:, :, :, self.zero_row] = 0.0
            else:
                self.a[:, self.zero_row, :, :k] = 0.0
            self.bias[:min(4, n)] = SPECIALS[:min(4, n)]
            self.bias[n - 1] = -1e-30
        self.dev_a, self.dev_b = D.from_host(self.a), D.from_host(self.b)
        self.g_bias = Guarded(1, n, (1, 1), n, 0, 0)
        self.g_bias.window()[...] = self.bias
        self.g_bias.upload(D)
        # float64 product of the valid parts, [b0, m, b1, n]
        a64, b64 = self.a[..., :d.a_shape[1]].astype(np.float64), self.b[..., :d.b_shape[1]].astype(np.float64)
        eq = ('zkhm' if case.layout == 'TN' else 'zmhk') + ',' + ('znhk' if case.layout == 'NT' else 'zkhn') + '->zmhn'
        self.prod64 = np.einsum(eq, a64, b64)
        window = dict(m=m, n=n, batch=batch, s0=d.sc[0], s1=d.sc[1])
        self.res = self.aux = self.rowvec = None
        if fam.flags & RESIDUAL:
            self.res = rng.standard_normal((batch[0], m, batch[1], n)).astype(np.float32)
            if not fam.alias:
                self.g_res = Guarded(ld=d.ldr, **window)
                self.g_res.window()[...] = self.res
                self.g_res.upload(D)
        if fam.flags & (RELU_MASK | SOFTMAX_BWD):
            self.aux = rng.standard_normal((batch[0], m, batch[1], n)).astype(np.float32)
            plant_specials(self.aux)
            self.g_aux = Guarded(ld=d.ldaux, **window)
            self.g_aux.window()[...] = self.aux
            self.g_aux.upload(D)
        if fam.flags & SOFTMAX_BWD:
            self.rowvec = rng.standard_normal((batch[0] * batch[1], m)).astype(np.float32)
            self.g_rowvec = Guarded(1, self.rowvec.size, (1, 1), self.rowvec.size, 0, 0)
            self.g_rowvec.window()[...] = self.rowvec.ravel()
            self.g_rowvec.upload(D)

    def rowvec_planes(self):
        """rowvec [b0 * b1, m] as [b0, m, b1, 1]."""
        b0, b1 = self.case.batch
        return self.rowvec.reshape(b0, b1, self.case.m).transpose(0, 2, 1)[..., None]


class Output(NamedTuple):
    c: np.ndarray                     # [b0, m, b1, n]
    aux: Optional[np.ndarray]         # the saved pre-activation (RELU_SAVE)
    colsum: Optional[np.ndarray]      # [b1, n]


def launch(ops: Operands, with_epilogue: bool) -> Output:
    """One launch of the case: with its epilogue, or (the plain run) with flags 0 and alpha 1 on the same operands, the same
    split and the same column-sum request.  C starts as sentinel NaNs (or as the residual where that aliases it); every guarded
    buffer is checked afterwards, inputs for their exact bits."""
    D, case, fam, d = ops.D, ops.case, ops.fam, ops.d
    m, n, k = case.m, case.n, case.k
    what = case.what + (' (epilogue run)' if with_epilogue else ' (plain run)')
    g_c = Guarded(m, n, case.batch, d.ldc, d.sc[0], d.sc[1])
    kwargs = dict(trans_a=case.layout == 'TN', trans_b=case.layout == 'NT', batch=case.batch, split_k=case.split_k)
    inputs = [ops.g_bias]
    g_save = g_sum = None
    if with_epilogue:
        kwargs['alpha'] = fam.alpha
        if fam.alias:
            g_c.window()[...] = ops.res
    g_c.upload(D)
    if with_epilogue:
        if fam.flags & BIAS:
            kwargs['bias'] = ops.g_bias.dev.flat_view(GUARD, [n])
        if fam.flags & RESIDUAL:
            kwargs['residual'] = g_c.mat(D) if fam.alias else ops.g_res.mat(D)
            inputs += [] if fam.alias else [ops.g_res]
        if fam.flags & RELU_SAVE:
            g_save = Guarded(m, n, case.batch, d.ldaux, d.sc[0], d.sc[1]).upload(D)
            kwargs['relu_save'] = g_save.mat(D)
        if fam.flags & RELU_MASK:
            kwargs['relu_mask'] = ops.g_aux.mat(D)
            inputs.append(ops.g_aux)
        if fam.flags & SOFTMAX_BWD:
            kwargs['softmax_bwd'] = (ops.g_aux.mat(D), ops.g_rowvec.dev.flat_view(GUARD, [ops.rowvec.size]))
            inputs += [ops.g_aux, ops.g_rowvec]
    if fam.colsum:
        g_sum = Guarded(1, case.batch[1] * n, (1, 1), case.batch[1] * n, 0, 0).upload(D)
        kwargs['colsum_out'] = g_sum.dev.flat_view(GUARD, [case.batch[1] * n])
    D.gemm(m, n, k, D.Mat(ops.dev_a, d.lda, *d.sa), D.Mat(ops.dev_b, d.ldb, *d.sb), g_c.mat(D), **kwargs)
    out = Output(g_c.download(what + ' C'), None if g_save is None else g_save.download(what + ' aux'),
                 None if g_sum is None else g_sum.download(what + ' colsum').reshape(case.batch[1], n))
    for g in inputs:
        g.unchanged(what)
    return out


# ---- references -------------------------------------------------------------------------------------------------------------------------
def epilogue(fam: Family, acc, bias, res, aux, rowvec, dtype):
    """(C, saved pre-activation or None) from accumulators [b0, m, b1, n] in ``dtype`` arithmetic, in the order of rmw_epilogue
    (csrc/npm_mfma_tile.h:244-253): alpha * acc, + bias, + residual, save / mask.  float32: the expression the device evaluates,
    rounding by rounding; float64: the value it approximates."""
    f = np.dtype(dtype).type
    acc = acc.astype(dtype)
    alpha = f(np.float32(fam.alpha))
    if fam.flags & SOFTMAX_BWD:
        return (alpha * aux.astype(dtype)) * (acc - rowvec.astype(dtype)), None
    v = acc if fam.alpha == 1.0 else alpha * acc
    if fam.flags & BIAS:
        v = v + bias.astype(dtype)
    if fam.flags & RESIDUAL:
        v = v + res.astype(dtype)
    pre = None
    if fam.flags & RELU_SAVE:
        pre = v
        v = np.maximum(v, f(0))
    if fam.flags & RELU_MASK:
        v = np.where(aux >= 0, v, f(0))
    return v, pre


def epilogue_loop(fam: Family, acc, bias, res, aux, rowvec):
    """``epilogue`` in float32, one element at a time in plain Python."""
    f = np.float32
    c, pre = np.empty(acc.shape, dtype=f), np.empty(acc.shape, dtype=f)
    alpha = f(fam.alpha)
    for z0, i, z1, j in np.ndindex(*acc.shape):
        a = f(acc[z0, i, z1, j])
        if fam.flags & SOFTMAX_BWD:
            c[z0, i, z1, j] = f(f(alpha * f(aux[z0, i, z1, j])) * f(a - f(rowvec[z0, i, z1, 0])))
            continue
        v = a if fam.alpha == 1.0 else f(alpha * a)
        if fam.flags & BIAS:
            v = f(v + f(bias[j]))
        if fam.flags & RESIDUAL:
            v = f(v + f(res[z0, i, z1, j]))
        if fam.flags & RELU_SAVE:
            pre[z0, i, z1, j] = v
            v = v if v > 0 else f(0)
        if fam.flags & RELU_MASK:
            v = v if aux[z0, i, z1, j] >= 0 else f(0)
        c[z0, i, z1, j] = v
    return c, (pre if fam.flags & RELU_SAVE else None)


def arm_of(fam: Family) -> str:
    """How the stored values are held to the float32 accumulators of the plain run.
    'equal'   -- alpha is 1, or there is no addend: every operation is one IEEE rounding (or none), so the bits are determined.
    'fma'     -- alpha * acc + addends: the compiler may contract the multiply-add, so |got - w| <= 3 * 2^-24 * (|alpha acc| + |bias|
                 + |res|) with w in float64: three roundings of intermediates no larger than that sum.
    'softmax' -- alpha * aux * (acc - rowvec): three roundings on two products and one difference, |got - w| <= 2^-22 |w|."""
    if fam.flags & SOFTMAX_BWD:
        return 'softmax'
    if fam.alpha != 1.0 and fam.flags & (BIAS | RESIDUAL):
        return 'fma'
    return 'equal'


def check(ops: Operands, plain: Output, got: Output, exact: bool, tol_plain: float = 2e-6, tol: float = 3e-6) -> None:
    """The assertions on one case.  The plain run against float64 (``tol_plain``, conftest.assert_close's metric); then, with
    ``exact``, the epilogue run against arithmetic on the plain run's accumulators (``arm_of``), otherwise against float64 at
    ``tol``; the column sums against the float64 column sums of the stored C."""
    case, fam = ops.case, ops.fam
    what = case.what
    assert_close(plain.c, ops.prod64, tol=tol_plain, what=what + ' (plain run)')
    rowvec = ops.rowvec_planes() if fam.flags & SOFTMAX_BWD else None
    if exact:
        arm = arm_of(fam)
        if arm == 'equal':
            want, pre = epilogue(fam, plain.c, ops.bias, ops.res, ops.aux, rowvec, np.float32)
            assert want.dtype == np.float32
            assert np.array_equal(got.c, want), f'{what}: C differs from the float32 expression on the accumulators at {_first(got.c, want)}'
            if pre is not None:
                assert np.array_equal(got.aux, pre), f'{what}: saved pre-activation differs at {_first(got.aux, pre)}'
        else:
            w, _ = epilogue(fam, plain.c, ops.bias, ops.res, ops.aux, rowvec, np.float64)
            if arm == 'fma':
                size = np.abs(np.float64(np.float32(fam.alpha)) * plain.c.astype(np.float64))
                size = size + (np.abs(ops.bias.astype(np.float64)) if fam.flags & BIAS else 0) + (np.abs(ops.res.astype(np.float64)) if fam.flags & RESIDUAL else 0)
                bound = 3 * 2.0 ** -24 * size
            else:
                bound = 2.0 ** -22 * np.abs(w)
            err = np.abs(got.c.astype(np.float64) - w)
            assert (err <= bound).all(), f'{what}: {arm} bound exceeded at {_first(err <= bound, True)}: err {err.max():.3e}'
    else:
        want, pre = epilogue(fam, ops.prod64, ops.bias, ops.res, ops.aux, rowvec, np.float64)
        assert_close(got.c, want, tol=tol, what=what)
        if pre is not None:
            assert_close(got.aux, pre, tol=tol, what=what + ' (saved pre-activation)')
    if fam.flags & RELU_SAVE:          # either way: C is the ReLU of what was saved, bit for bit
        assert np.array_equal(got.c, np.maximum(got.aux, np.float32(0))), what + ': C is not max(aux, 0)'
    if fam.colsum:
        for out in (plain, got):
            assert_close(out.colsum, out.c.astype(np.float64).sum(axis=(0, 1)), tol=3e-6, what=what + ' (column sums)')


def _first(a, b):
    bad = np.argwhere(~(np.asarray(a) == np.asarray(b)))
    return None if not len(bad) else (tuple(int(i) for i in bad[0]), len(bad))
