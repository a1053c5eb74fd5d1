"""TEST INFRASTRUCTURE ONLY -- the Conv2D path tests: the dispatch of np_modeling_amd/csrc/npm_conv.hip (the conv plans of
csrc/npm_gemm_plan.h) restated (``route``), the
fixed case lists with the cell each case exists for, the geometry properties those cells claim (computed, so that
tests/test_conv_host.py can prove them on the CPU) and the harness that runs a case on the device (``ConvCall``).
tests/test_gpu_conv_paths.py runs the same lists on the GPU and asserts that ``npm_last_conv_kernel`` reports what ``route`` says.

A *cell* is what a case is there for: a kernel instance at a geometry class, a knob value, an epilogue, a fallback reason.
Shapes are the smallest that have the property.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

BM = BN = 128
BK = 32                    # K tile of the register-staged kernels
GK = 16                    # K tile of the LDS-DMA kernels: one 16-pixel piece
# include/npm_hip.h NPM_TUNE_*
TUNE_CONV_DMA, TUNE_WGRAD_BLOCKS, TUNE_WAVE_PRIO, TUNE_WGRAD_FUSED, TUNE_KSYNC, TUNE_KORDER = 4, 8, 9, 13, 15, 16
E_BAD_ARGUMENT = 10002
# npm_set_math mode -> (what the conv kernels run: npm_conv_set_math, csrc/npm_gemm.hip NPM_TUNE_GEMM_MATH; what npm_last_math says)
CONV_MATH = {'f32': (0, 'f32'), 'bf16x3_fast': (1, 'bf16x3_fast'), 'bf16x3': (2, 'bf16x3'), 'f16x2': (2, 'bf16x3')}


class Knobs(NamedTuple):
    dma: int = 1               # NPM_TUNE_CONV_DMA
    korder: int = 1            # NPM_TUNE_CONV_KORDER
    prio: int = 0              # NPM_TUNE_GEMM_WAVE_PRIO
    blocks: int = 0            # NPM_TUNE_CONV_WGRAD_BLOCKS
    fused: int = 1             # NPM_TUNE_CONV_WGRAD_FUSED
    ksync: int = 128           # NPM_TUNE_KSYNC
    math: str = 'f32'          # npm_set_math

    @property
    def tag(self):
        return '-'.join(f'{k}{v}' for k, v in self._asdict().items() if v != getattr(DEFAULT, k)) or 'default'


DEFAULT = Knobs()


# ---- the dispatch, restated -------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def pick_splits(tiles, nkt, cus, force_per_cu=0, resident=4):
    """csrc/npm_gemm_plan.h pick_splits with generations = 0 (the conv entry points never pass it)."""
    max_s = nkt // 8
    if force_per_cu > resident:
        s = force_per_cu * cus // tiles
        return 1 if s < 1 else max_s if s > max_s else s
    best, best_cost = 1, 1e30
    first = resident if resident < 3 else 3
    second = resident - 1 if first == resident else resident
    for per_cu in (first, first if second < 2 else second):
        if 0 < force_per_cu <= resident and per_cu != force_per_cu:
            continue
        s = max(1, min(per_cu * cus // tiles, max_s))
        cost = float(_cdiv(tiles * s, cus)) / float(s)
        if cost < best_cost * (1.0 - 1e-6):
            best_cost, best = cost, s
    return best


def _fmt(family, vec, tall, math, korder, buf, splits, kper, wr=0, trio=False, ksync=0):
    return '%s vec=%d tall=%d math=%d korder=%d buf=%d splits=%d kper=%d wr=%d trio=%d ksync=%d' % (
        family, vec, tall, math, korder, buf, splits, kper, wr, trio, ksync)


def _route_gemm(n, h, w, c, n_out, k, kn, aligned):
    """conv_gemm_plan: forward (c = c_in, n_out = c_out) and grad_x (c = c_out, n_out = c_in)."""
    if n == 0:
        return 'none'
    math = CONV_MATH[kn.math][0]
    pad = k // 2
    halo = pad * w + pad
    kk = k * k * c
    vec = c % 4 == 0 and n_out % 4 == 0 and aligned
    buf_ok = bool(kn.dma) and (256 * n_out + n_out) * 4 < 2 ** 31
    dma = bool(kn.dma) and vec and c % GK == 0 and (256 + 2 * halo) * c * 4 < 2 ** 30 and kk * n_out * 4 < 2 ** 31
    tall = dma and n_out <= 64 and n_out % 16 == 0 and kn.dma != 2
    return _fmt('conv_fwd_glds' if dma else 'conv_fwd', vec, tall, math if dma else 0, kn.korder if dma else 0, dma and buf_ok, 1, kk)


def _renormalise(nkt, splits):
    """csrc/npm_gemm_plan.h split_ranges, as the conv entry points see it (nkt >= 1)."""
    splits = max(1, splits)
    kt_per = _cdiv(nkt, splits)
    return _cdiv(nkt, kt_per), kt_per


def _route_bwd_w(n, h, w, c0, c1, k, kn, cus, aligned):
    """conv_wgrad_plan: the filter gradient."""
    pixels = n * h * w
    if pixels == 0:
        return 'none'
    math = CONV_MATH[kn.math][0]
    halo = (k // 2) * w + k // 2
    tiles = _cdiv(k * k * c0, BM) * _cdiv(c1, BN)
    nkt = _cdiv(pixels, BK)
    splits = 1
    if tiles < 2 * cus and nkt >= 16:
        if kn.blocks < 0:
            splits = min(_cdiv(3 * cus, tiles), nkt // 8)
        else:
            splits = pick_splits(tiles, nkt, cus, kn.blocks, {2: 2, 1: 3, 0: 4}[math])
    splits, kt_per = _renormalise(nkt, splits)
    kper = kt_per * BK
    vec = c0 % 4 == 0 and c1 % 4 == 0 and aligned
    buf_ok = bool(kn.dma) and (256 * c1 + c1) * 4 < 2 ** 31
    dma = (bool(kn.dma) and vec and pixels % GK == 0 and kper % GK == 0 and (kper + 2 * halo + GK) * c0 * 4 < 2 ** 30
           and kper * c1 * 4 < 2 ** 30)
    return _fmt('conv_wgrad_glds' if dma else 'conv_wgrad', vec, False, math if dma else 0, 0, dma and buf_ok, splits, kper)


def ksync_every(value):
    """npm::set_ksync_every: a power of two, or off."""
    return value if value > 0 and value & (value - 1) == 0 else 0


def fused_plan(n, h, w, c0, c1, k, kn, cus, aligned=True):
    """conv_wgrad_fused_plan (npm_conv2d_bwd_w_relu's choices) as a dict, or None where it takes the two-pass form."""
    pixels, m = n * h * w, k * k * c0
    halo = (k // 2) * w + k // 2
    fused = (bool(kn.dma) and CONV_MATH[kn.math][0] == 0 and bool(kn.fused) and c0 % 4 == 0 and c1 % 4 == 0 and pixels % GK == 0
             and w >= GK and aligned and m * c1 * 4 < 2 ** 31)
    if not fused:
        return None
    pad128, pad192 = _cdiv(m, 128) * 128, _cdiv(m, 192) * 192
    tall = kn.fused == 3 or (kn.fused != 2 and pad192 < pad128)
    rows, resident = (192, 3) if tall else (128, 4)
    tiles_m, tiles_n = _cdiv(m, rows), _cdiv(c1, BN)
    tiles = tiles_m * tiles_n
    nkt = pixels // GK
    splits = 1
    if tiles < 2 * cus and nkt >= 16:
        splits = pick_splits(tiles, nkt, cus, kn.blocks if kn.blocks > 0 else 0, resident)
    splits, kt_per = _renormalise(nkt, splits)
    kper = kt_per * GK
    if not ((kper + 2 * halo + GK) * c0 * 4 < 2 ** 30 and kper * c1 * 4 < 2 ** 30 and tiles * splits < 2 ** 31):
        return None
    trio = tall and tiles_m == 3 and splits > 1 and kn.fused != 3
    grid = (tiles_n if trio else tiles) * splits
    every = ksync_every(kn.ksync)
    engaged = not trio and splits > 1 and grid <= resident * cus and every > 0 and kt_per >= 2 * every
    return dict(rows=rows, tiles_m=tiles_m, tiles_n=tiles_n, nkt=nkt, splits=splits, kt_per=kt_per, kper=kper, trio=trio,
                ksync=every if engaged else 0, last_rows=m - (tiles_m - 1) * rows)


def route(entry, n, h, w, c0, c1, k, knobs=DEFAULT, cus=256, aligned=True):
    """The string ``npm_last_conv_kernel`` must report after ``entry`` ('fwd', 'bwd_x', 'bwd_w', 'bwd_w_relu') on this shape
    with these knobs on a device of ``cus`` compute units; ``aligned``: every tensor the vec test looks at starts on 16 bytes."""
    if entry == 'fwd':
        return _route_gemm(n, h, w, c0, c1, k, knobs, aligned)
    if entry == 'bwd_x':                  # the flipped filter is the library's own allocation: aligned
        return _route_gemm(n, h, w, c1, c0, k, knobs, aligned)
    if entry == 'bwd_w':
        return _route_bwd_w(n, h, w, c0, c1, k, knobs, cus, aligned)
    assert entry == 'bwd_w_relu', entry
    if n * h * w == 0:
        return 'none'
    plan = fused_plan(n, h, w, c0, c1, k, knobs, cus, aligned)
    if plan is None:
        return 'two_pass ' + _route_bwd_w(n, h, w, c0, c1, k, knobs, cus, aligned)
    return _fmt('conv_wgrad_relu', True, False, 0, 0, True, plan['splits'], plan['kper'], plan['rows'] // 64, plan['trio'], plan['ksync'])


def fields(report: str) -> dict:
    words = report.split()
    two_pass = words[0] == 'two_pass'
    words = words[1:] if two_pass else words
    out = dict(family=words[0], two_pass=two_pass)
    out.update((key, int(value)) for key, value in (word.split('=') for word in words[1:]))
    return out


def instance(report: str) -> str:
    """'scalar' / 'vec' (register-staged), 'dma' (LDS-DMA 128 x 128), 'tall' (LDS-DMA 256 x 64), 'fused', 'none'."""
    if report == 'none':
        return 'none'
    f = fields(report)
    if f['family'] == 'conv_wgrad_relu':
        return 'fused'
    if f['family'].endswith('_glds'):
        return 'tall' if f['tall'] else 'dma'
    return 'vec' if f['vec'] else 'scalar'


# ---- fast_div, restated with Python integers -----------------------------------------------------------------------------------------------
def fast_div_setup(d):
    """csrc/npm_conv.hip fast_div_setup: (mul, shift) of 32 bits each."""
    lg = 0
    while (1 << lg) < d:
        lg += 1
    k = 31 + lg
    mul = ((1 << k) + d - 1) // d
    if d == 1:
        return 0, 0
    assert mul < 2 ** 32 and k >= 32
    return mul, k - 32


def fast_div(n, d, mul, shift):
    return n if d == 1 else ((n * mul) >> 32) >> shift


# ---- geometry properties ---------------------------------------------------------------------------------------------------------------
def piece_images(n, h, w):
    """Per 16-pixel piece of the forward / grad_x gather: how many images its valid pixels lie in."""
    m = n * h * w
    return [(min(p + 15, m - 1)) // (h * w) - p // (h * w) + 1 for p in range(0, m, 16)]


def piece_rows(n, h, w):
    """Per 16-pixel piece: how many image rows its valid pixels touch."""
    m = n * h * w
    return [min(p + 15, m - 1) // w - p // w + 1 for p in range(0, m, 16)]


def piece_is_fast(n, h, w, k, p):
    """The piece starting at pixel p has at least one tap for which conv_fwd_glds_kernel skips the per-lane test."""
    m, pad = n * h * w, k // 2
    pwf, phf = p % w, (p // w) % h
    if not (k <= 31 and pwf + 15 < w and p + 15 < m):
        return False
    hm = any(0 <= phf + t - pad < h for t in range(k))
    wm = any(pwf + t - pad >= 0 and pwf + 15 + t - pad < w for t in range(k))
    return hm and wm


def interior_tiles(n, h, w, k):
    """Per K tile of the fused filter gradient (16 pixels): the ``interior`` test of NPM_WGRAD_ISSUE."""
    pad = k // 2
    out = []
    for p in range(0, n * h * w, GK):
        w0, h0 = p % w, (p // w) % h
        out.append(w0 + GK <= w - pad and w0 >= pad and h0 >= pad and h0 < h - pad)
    return out


def seams(pixels, splits, kper):
    return [s * kper for s in range(1, splits)]


GEOMETRY_CLAIMS = {
    # class -> predicate on (n, h, w, k)
    'w1': lambda n, h, w, k: w == 1 and h == 1 and fast_div_setup(w) == (0, 0),
    'h1_straddle_midpiece': lambda n, h, w, k: h == 1 and max(piece_images(n, h, w)) >= 2 and (n * h * w) % 16 != 0,
    'smaller_than_reach': lambda n, h, w, k: h <= k // 2 and w <= k // 2 and max(piece_images(n, h, w)) >= 3,
    'narrow_five_rows': lambda n, h, w, k: w <= k // 2 + 1 and max(piece_rows(n, h, w)) >= 5,      # no column has both neighbours of a 5-tap row
    'm240': lambda n, h, w, k: 128 < n * h * w < 256 and (n * h * w) % 128 != 0,
    'w16': lambda n, h, w, k: w == 16 and any(piece_is_fast(n, h, w, k, p) for p in range(0, n * h * w, 16)),
    'wrap_mixed': lambda n, h, w, k: (w % 16 != 0 and any(piece_is_fast(n, h, w, k, p) for p in range(0, n * h * w, 16))
                                      and any(r == 2 for r in piece_rows(n, h, w))),
    'prime_wide': lambda n, h, w, k: w > 128 and all(w % q for q in range(2, w)),
    'm429': lambda n, h, w, k: n * h * w > 256 and (n * h * w) % 16 != 0 and _cdiv(n * h * w, 128) == 4 and _cdiv(n * h * w, 256) == 2,
}

# (class, (n, h, w, k)): what the class pins is in GEOMETRY_CLAIMS
FWD_GEOMETRIES = [
    ('w1', (16, 1, 1, 3)),                        # every pixel its own image, W = 1: fast_div's d == 1 path
    ('h1_straddle_midpiece', (5, 1, 17, 3)),      # H = 1, pieces straddle images, M = 85 ends mid-piece
    ('smaller_than_reach', (3, 2, 2, 7)),         # image smaller than the reach
    ('narrow_five_rows', (2, 9, 3, 5)),           # W < pad + 1, five rows per piece
    ('m240', (1, 20, 12, 3)),                     # one tall tile, two square ones, the second ragged
    ('w16', (2, 7, 16, 5)),                       # W = 16 exactly
    ('wrap_mixed', (1, 5, 37, 3)),                # pieces wrap mid-row, fast and border pieces mixed
    ('prime_wide', (1, 3, 131, 3)),               # prime W wider than a tile
    ('m429', (3, 11, 13, 3)),
]
# (c_in, c_out) -> (forward's instance, grad_x's instance)
CHANNELS = {
    (3, 5): ('scalar', 'scalar'),
    (4, 8): ('vec', 'vec'),
    (20, 12): ('vec', 'vec'),
    (16, 132): ('dma', 'vec'),                    # two column tiles, the second ragged
    (32, 68): ('dma', 'vec'),                     # N <= 128, not a multiple of 16
    (68, 32): ('vec', 'dma'),                     # grad_x on the square DMA tile
    (16, 16): ('tall', 'tall'),
    (32, 64): ('tall', 'tall'),
    (16, 48): ('tall', 'tall'),                   # 48 of 64 columns
}
DMA_CHANNELS = [c for c, inst in CHANNELS.items() if set(inst) & {'dma', 'tall'}]
# forward epilogues: (name, bias, relu, pre saved)
EPILOGUES = [('bias_relu_pre', True, 1, True), ('relu', False, 1, False), ('bias', True, 0, False), ('none', False, 0, False)]


class FwdCase(NamedTuple):
    geometry: str
    n: int
    h: int
    w: int
    k: int
    c0: int
    c1: int
    knobs: Knobs = DEFAULT
    offset: int = 0            # floats the gathered tensors' base is shifted off 16-byte alignment
    cell: str = ''             # for the knob / alignment cases: what the case is there for

    @property
    def id(self):
        return f'{self.geometry}-{self.c0}x{self.c1}-{self.knobs.tag}' + ('-off%d' % self.offset if self.offset else '')

    @property
    def shape(self):
        return self.n, self.h, self.w, self.c0, self.c1, self.k

    def routes(self, cus=256, math=None):
        kn = self.knobs if math is None else self.knobs._replace(math=math)
        return tuple(route(e, *self.shape, kn, cus, aligned=not self.offset) for e in ('fwd', 'bwd_x'))


def _fwd(geometry, shape, channels, **kw):
    n, h, w, k = shape
    return FwdCase(geometry, n, h, w, k, channels[0], channels[1], **kw)


FWD_PLAIN = [_fwd(g, s, c) for g, s in FWD_GEOMETRIES for c in CHANNELS if c not in DMA_CHANNELS]        # f32 only
FWD_DMA = [_fwd(g, s, c) for g, s in FWD_GEOMETRIES for c in DMA_CHANNELS]                                # every math mode
# Knobs, on channel pairs with two 16-channel chunks (with one chunk both K orders are the same walk): (32, 68) forward on the
# square tile, (32, 64) both directions on the tall one.  CONV_DMA = 2 only where it changes the route (N <= 64).
FWD_KNOBS = ([_fwd(g, s, c, knobs=Knobs(korder=0), cell='korder0') for g, s in FWD_GEOMETRIES for c in ((32, 68), (32, 64))]
             + [_fwd(g, s, c, knobs=Knobs(dma=0), cell='dma0') for g, s in FWD_GEOMETRIES for c in ((32, 68), (32, 64))]
             + [_fwd(g, s, (32, 64), knobs=Knobs(dma=2), cell='dma2') for g, s in FWD_GEOMETRIES])
FWD_PRIO = [_fwd(g, s, c, knobs=Knobs(prio=p), cell='prio%d' % p) for g, s in FWD_GEOMETRIES[1::3] for c in ((32, 68), (32, 64))
            for p in (1, 2, 3)]
# a base 4 bytes off alignment forces the scalar instance at vec-friendly and at DMA-eligible channel counts
FWD_MISALIGNED = [_fwd(g, s, c, offset=1, cell='misaligned') for g, s in (FWD_GEOMETRIES[1], FWD_GEOMETRIES[4], FWD_GEOMETRIES[8])
                  for c in ((4, 8), (32, 64))]


# ---- filter gradient ------------------------------------------------------------------------------------------------------------------
class WgradCase(NamedTuple):
    cell: str
    n: int
    h: int
    w: int
    c0: int
    c1: int
    k: int
    knobs: Knobs = DEFAULT
    offset: int = 0
    cus_dependent: bool = False          # the split count moves with the device's CU count: asserted through the device's own
    expect: str = 'dma'                  # instance at 256 CUs

    @property
    def id(self):
        return f'{self.cell}-{self.n}x{self.h}x{self.w}-{self.c0}x{self.c1}-k{self.k}-{self.knobs.tag}' + ('-off1' if self.offset else '')

    @property
    def shape(self):
        return self.n, self.h, self.w, self.c0, self.c1, self.k

    def route(self, cus=256, math=None, entry='bwd_w'):
        kn = self.knobs if math is None else self.knobs._replace(math=math)
        return route(entry, *self.shape, kn, cus, aligned=not self.offset)


WGRAD_DMA = [
    WgradCase('one_ktile', 16, 1, 1, 16, 16, 3),                  # W = 1: dh_ = 16 and the `while (ph >= H)` loop
    WgradCase('w1_three_ktiles', 48, 1, 1, 16, 16, 3),            # the same over three K tiles: (h, w) advance by sixteen images a tile
    WgradCase('w2_h1', 8, 1, 2, 8, 20, 3),
    WgradCase('w2', 16, 3, 2, 16, 132, 3),
    WgradCase('w3', 4, 4, 3, 4, 8, 3),
    WgradCase('k7_w8', 4, 5, 8, 8, 16, 7),
    WgradCase('m240', 2, 20, 12, 64, 128, 3),
    WgradCase('split_seam', 1, 16, 31, 16, 20, 3),                # 496 pixels: 16 K tiles of 32, two splits of 256 and 240 pixels
    WgradCase('one_split', 1, 16, 30, 16, 20, 3),                 # 480 pixels: 15 K tiles, one split
] + [WgradCase('split_seam_blocks', 1, 16, 31, 16, 20, 3, Knobs(blocks=b)) for b in (-1, 3, 4, 6, 12)] + [
    # 25 output tiles over 512 K tiles: every WGRAD_BLOCKS value is another split count (29, 31, 40, 57, 64 at 256 CUs)
    WgradCase('many_tiles_blocks', 4, 64, 64, 64, 16, 7, Knobs(blocks=b), cus_dependent=True) for b in (0, -1, 3, 4, 6, 12)]
WGRAD_PLAIN = [
    WgradCase('pixels_not_16', 3, 11, 13, 8, 12, 3, expect='vec'),
    WgradCase('scalar_channels', 1, 16, 31, 3, 5, 3, expect='scalar'),
    WgradCase('scalar_channels_k5', 2, 9, 3, 6, 4, 5, expect='scalar'),
    WgradCase('dma0', 1, 16, 31, 16, 20, 3, Knobs(dma=0), expect='vec'),
    WgradCase('misaligned', 1, 16, 31, 16, 20, 3, offset=1, expect='scalar'),
]


# ---- fused filter gradient ---------------------------------------------------------------------------------------------------------------
FUSED_GEOMETRIES = [
    ('h1', (16, 1, 17, 3)),                  # H = 1
    ('h_eq_pad', (2, 2, 16, 5)),             # H = pad: no interior tile
    ('seam_in_row', (1, 16, 31, 3)),
    ('k7', (4, 3, 20, 7)),
    ('odd_ktiles', (1, 33, 16, 3)),          # 33 K tiles: odd count, uneven splits
]
FUSED_CLAIMS = {
    'h1': lambda n, h, w, k: h == 1 and not any(interior_tiles(n, h, w, k)),
    'h_eq_pad': lambda n, h, w, k: h == k // 2 and not any(interior_tiles(n, h, w, k)),
    'seam_in_row': lambda n, h, w, k: any(interior_tiles(n, h, w, k)) and not all(interior_tiles(n, h, w, k)) and w % GK != 0,
    'k7': lambda n, h, w, k: k == 7 and h == k // 2 and (n * h * w) // GK < 16,
    'odd_ktiles': lambda n, h, w, k: ((n * h * w) // GK) % 2 == 1 and (n * h * w) // GK >= 32,
}
# c_in per kernel size, by the tiling k*k*c_in takes (at the default knob unless forced)
FUSED_CIN = {3: (8, 16, 32, 64), 5: (4, 8, 36), 7: (4, 12)}
FUSED_COUT = (4, 20, 132)


def tiling_class(n, h, w, c0, c1, k, knobs=DEFAULT, cus=256):
    """'128x<rows>' / '192x<rows>' / 'trio', '+ragged<r>' when the last tile row holds r < tile height rows; None off the fused path."""
    plan = fused_plan(n, h, w, c0, c1, k, knobs, cus)
    if plan is None:
        return None
    name = 'trio' if plan['trio'] else '%dx%d' % (plan['rows'], plan['tiles_m'])
    return name + ('+ragged%d' % plan['last_rows'] if plan['last_rows'] != plan['rows'] else '')


class FusedCase(NamedTuple):
    cell: str
    n: int
    h: int
    w: int
    c0: int
    c1: int
    k: int
    knobs: Knobs = DEFAULT
    offset: int = 0
    cus_dependent: bool = False

    @property
    def id(self):
        return f'{self.cell}-{self.n}x{self.h}x{self.w}-{self.c0}x{self.c1}-k{self.k}-{self.knobs.tag}' + ('-off1' if self.offset else '')

    @property
    def shape(self):
        return self.n, self.h, self.w, self.c0, self.c1, self.k

    def route(self, cus=256):
        return route('bwd_w_relu', *self.shape, self.knobs, cus, aligned=not self.offset)


def _fused_cases():
    """Every geometry x c_in of its kernel size, c_out rotating; under WGRAD_FUSED 1, 2, 3, 0 wherever that changes the route."""
    out, i = [], 0
    for geometry, (n, h, w, k) in FUSED_GEOMETRIES:
        for c0 in FUSED_CIN[k]:
            c1 = FUSED_COUT[i % 3]
            i += 1
            seen = set()
            for mode in (1, 2, 3, 0):
                kn = Knobs(fused=mode)
                r = route('bwd_w_relu', n, h, w, c0, c1, k, kn)
                if r in seen:
                    continue
                seen.add(r)
                out.append(FusedCase(geometry, n, h, w, c0, c1, k, kn))
    return out


FUSED = _fused_cases()
# one case per reason for the two-pass form
FUSED_FALLBACK = [
    FusedCase('w15', 2, 16, 15, 8, 20, 3),
    FusedCase('pixels_not_16', 1, 5, 17, 8, 20, 3),
    FusedCase('channels_not_4', 1, 16, 31, 6, 20, 3),
    FusedCase('cout_not_4', 1, 16, 31, 8, 5, 3),
    FusedCase('math', 1, 16, 31, 16, 20, 3, Knobs(math='bf16x3')),
    FusedCase('dma0', 1, 16, 31, 16, 20, 3, Knobs(dma=0)),
    FusedCase('misaligned', 1, 16, 31, 16, 20, 3, offset=1),
]
# The K rendezvous at a small size: 1024 K tiles over 128 splits of 8 (256 CUs), three four-wave blocks per split
RENDEZVOUS_SHAPE = (4, 64, 64, 64, 128, 3)
RENDEZVOUS_KSYNC = (0, 2, 4)


# ---- the harness ---------------------------------------------------------------------------------------------------------------------------
GUARD = 64                                                     # floats on each side of every output
POISON = np.uint32(0x7FC00BAD).view(np.float32)                # around the inputs: a quiet NaN, shows in whatever sum it reaches
UNWRITTEN = np.uint32(0x7FC00777).view(np.float32)             # pre-fill of every output element
FENCE = np.uint32(0x7FC00999).view(np.float32)                 # the guard words of the outputs
SPECIALS = np.array([0.0, -0.0, 1e-30, -1e-30], dtype=np.float32)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


class Input:
    """[poison | tensor | poison] on the device; ``ptr`` is the tensor's base, ``offset`` floats off 16-byte alignment."""

    def __init__(self, D, value: np.ndarray, margin: int, offset: int = 0):
        margin = _cdiv(max(margin, GUARD), 4) * 4
        flat = np.full(2 * margin + 4 + value.size, POISON, dtype=np.float32)
        flat[margin + offset:margin + offset + value.size] = value.ravel()
        self.dev = D.from_host(flat)
        assert self.dev.ptr % 16 == 0
        self.ptr = self.dev.ptr + 4 * (margin + offset)


class Output:
    """[fence | unwritten ... | fence] on the device.  ``read`` returns the tensor and checks that every fence word survived and
    that no element kept its pre-fill."""

    def __init__(self, D, shape):
        self.shape, self.size = tuple(shape), int(np.prod(shape))
        self.flat = np.full(2 * GUARD + self.size, FENCE, dtype=np.float32)
        self.flat[GUARD:GUARD + self.size] = UNWRITTEN
        self.dev = D.from_host(self.flat)
        self.ptr = self.dev.ptr + 4 * GUARD

    def raw(self):
        return self.dev.numpy()

    def read(self, what, written=True):
        flat = self.raw()
        for side, part in (('front', slice(0, GUARD)), ('back', slice(GUARD + self.size, None))):
            assert np.array_equal(bits(flat[part]), bits(self.flat[part])), f'{what}: a guard word {side} of the tensor was written'
        body = flat[GUARD:GUARD + self.size].reshape(self.shape).copy()
        if written:
            left = int((bits(body) == bits(UNWRITTEN)).sum())
            assert left == 0, f'{what}: {left} of {self.size} elements were never written'
            assert not np.isnan(body).any(), f'{what}: NaN in the result (memory outside an input was read)'
        else:
            assert (bits(body) == bits(UNWRITTEN)).all(), f'{what}: written'
        return body


class ConvCall:
    """One shape's operands on the device and the four entry points on them.  x, dy, pre and the filter sit inside poison, every
    output inside fences and pre-filled; knobs are set for one call and restored whatever happens."""

    def __init__(self, D, _C, shape, seed, offset=0, specials=True):
        self.D, self._C, self.lib = D, _C, _C.lib()
        n, h, w, c0, c1, k = self.shape = shape
        rng = np.random.default_rng([seed, n, h, w, c0, c1, k])
        self.x = rng.standard_normal((n, h, w, c0)).astype(np.float32)
        self.filt = rng.standard_normal((k, k, c0, c1)).astype(np.float32)
        self.bias = rng.standard_normal(c1).astype(np.float32)
        self.dy = rng.standard_normal((n, h, w, c1)).astype(np.float32)
        self.pre = rng.standard_normal((n, h, w, c1)).astype(np.float32)
        if specials:                                    # the mask is pre >= 0: +0, -0 and +-1e-30, first and last elements included
            flat = self.pre.reshape(-1)
            flat[::7] = np.resize(SPECIALS, flat[::7].size)
            head = min(4, flat.size)
            flat[:head] = SPECIALS[:head]
            flat[-1] = -0.0
        reach = ((k // 2) * w + k // 2 + GK)            # pixels a wrong tap could reach outside the tensor
        self.d_x = Input(D, self.x, reach * c0, offset)
        self.d_dy = Input(D, self.dy, reach * c1, offset)
        self.d_pre = Input(D, self.pre, reach * c1)
        self.d_filt = Input(D, self.filt, GUARD)
        self.d_bias = Input(D, self.bias, GUARD)

    def _tuned(self, knobs: Knobs):
        return _Tuned(self._C, knobs)

    def fwd(self, knobs=DEFAULT, bias=True, relu=1, save_pre=True):
        """-> (y, pre or None, report, last_math)"""
        n, h, w, c0, c1, k = self.shape
        y, pre = Output(self.D, (n, h, w, c1)), Output(self.D, (n, h, w, c1)) if save_pre else None
        desc = self._C.npm_conv2d(n=n, h=h, w=w, c_in=c0, c_out=c1, ksize=k, x=self.d_x.ptr, filt=self.d_filt.ptr,
                                  bias=self.d_bias.ptr if bias else None, y=y.ptr, pre=pre.ptr if save_pre else None, relu=relu)
        import ctypes
        with self._tuned(knobs):
            self._C.check(self.lib.npm_conv2d_fwd(ctypes.byref(desc)), 'npm_conv2d_fwd')
            report, math = self._C.last_conv_kernel(), self._C.last_math()
        return y.read('y'), (pre.read('pre') if save_pre else None), report, math

    def bwd_x(self, knobs=DEFAULT):
        n, h, w, c0, c1, k = self.shape
        dx = Output(self.D, (n, h, w, c0))
        with self._tuned(knobs):
            self._C.check(self.lib.npm_conv2d_bwd_x(self.d_dy.ptr, self.d_filt.ptr, dx.ptr, n, h, w, c0, c1, k), 'npm_conv2d_bwd_x')
            report, math = self._C.last_conv_kernel(), self._C.last_math()
        return dx.read('dx'), report, math

    def bwd_w(self, knobs=DEFAULT):
        n, h, w, c0, c1, k = self.shape
        dw = Output(self.D, (k, k, c0, c1))
        with self._tuned(knobs):
            self._C.check(self.lib.npm_conv2d_bwd_w(self.d_dy.ptr, self.d_x.ptr, dw.ptr, n, h, w, c0, c1, k), 'npm_conv2d_bwd_w')
            report, math = self._C.last_conv_kernel(), self._C.last_math()
        return dw.read('dw'), report, math

    def bwd_w_relu(self, knobs=DEFAULT):
        """-> (g, dw, db, report)"""
        n, h, w, c0, c1, k = self.shape
        g, dw, db = Output(self.D, (n, h, w, c1)), Output(self.D, (k, k, c0, c1)), Output(self.D, (c1,))
        with self._tuned(knobs):
            self._C.check(self.lib.npm_conv2d_bwd_w_relu(self.d_dy.ptr, self.d_pre.ptr, self.d_x.ptr, g.ptr, dw.ptr, db.ptr,
                                                         n, h, w, c0, c1, k), 'npm_conv2d_bwd_w_relu')
            report = self._C.last_conv_kernel()
        return g.read('g'), dw.read('dw'), db.read('db'), report


class _Tuned:
    """The six conv knobs and the math mode for the duration of a ``with`` block, defaults afterwards."""

    IDS = dict(dma=TUNE_CONV_DMA, korder=TUNE_KORDER, prio=TUNE_WAVE_PRIO, blocks=TUNE_WGRAD_BLOCKS, fused=TUNE_WGRAD_FUSED,
               ksync=TUNE_KSYNC)

    def __init__(self, _C, knobs: Knobs):
        self._C, self.knobs = _C, knobs

    def _set(self, knobs):
        lib = self._C.lib()
        for name, knob in self.IDS.items():
            self._C.check(lib.npm_set_tuning(knob, getattr(knobs, name)), 'npm_set_tuning')

    def __enter__(self):
        self.math_before = self._C.get_math()
        try:
            self._set(self.knobs)
            if self.knobs.math != DEFAULT.math:
                self._C.set_math(self.knobs.math)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        self._set(DEFAULT)
        if self._C.get_math() != self.math_before:
            self._C.set_math(self.math_before)
        return False
