"""MI355X: half-precision weight copies -- the conversions (npm_cvt_f32_f16 / npm_cvt_f16_f32), the skinny-M GEMM over fp16
weights (npm_sgemm_skinny_w16, csrc/npm_skinny.hip) and the layers that use them.

Bounds.  The kernel is tested against float64 NumPy ON THE ROUNDED WEIGHTS (w.astype(float16).astype(float32): the conversion
in registers is exact) within tests/skinny_cases.py TOL = 2e-6 in conftest.assert_close's metric; the derivation in
tests/test_gpu_skinny.py's docstring carries over unchanged, since the fp32 chain behind the conversion is the same one: at least
four partial sums per element.  The distance from the product on the ORIGINAL weights is bounded elementwise by
2^-11 sum_k |a_k w_k| (half rounding of normal weights: relative 2^-11) + 2^-25 sum_k |a_k| (of weights whose halves are
subnormal: absolute 2^-25) + TOL (|y32| + max |y32|) (the two fp32 summations).  Layers: LAYER_TOL = 1e-5 against
tests/decode_reference.py on the rounded parameters and 2 LAYER_TOL against the same layer holding the rounded values as floats.
Every test prints the fraction of its bound it used before it asserts.
"""

import ctypes as C

import numpy as np
import pytest

import decode_cases as DC
import decode_reference as DR
import skinny_cases as SC
import varlen_reference as VR
from conftest import assert_close

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 777.0
HALF_SENTINEL = 0x5E17                                                    # a finite half that no test value rounds to by design
SPLITS_KNOB, NT_KNOB = 22, 23
UNSUPPORTED, BAD_ARGUMENT = 10003, 10002
SHAPES = ((16, 16), (48, 32), (272, 528), (1024, 1024))                  # (N, K): one chunk; a narrow strip; ragged strip, 33 chunks; 8 splits
ROWS = (1, 15, 16, 17, 33, 64)
ALPHAS = (1.0, 0.37, -1.5)
SIX = (('_self_attention', '_wq'), ('_self_attention', '_wk'), ('_self_attention', '_wv'), ('_self_attention', '_wo'),
       ('_cross_attention', '_wq'), ('_cross_attention', '_wo'), ('_dense1._linear', '_w'), ('_dense2', '_w'))


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


def _tune(knob, value):
    from np_modeling_amd import _C
    _C.check(_C.lib().npm_set_tuning(knob, int(value)), 'npm_set_tuning')


def _rounded(w):
    with np.errstate(over='ignore'):
        return np.asarray(w, dtype=np.float32).astype(np.float16).astype(np.float32)


_WEIGHTS = {}


def _weights(layout, n, k, seed=0):
    """B of one (layout, N, K), once per process: N(0, 1) / sqrt(K) floats, and on the device both as floats and as halves, rows 8
    elements wider than the matrix and, for NT, one more row than N; everything outside the matrix is NaN (fp32 NaN / fp16 NaN).
    Returns (host floats, host rounded floats, device floats, device halves, ldb)."""
    from np_modeling_amd import device as D
    key = (layout, n, k, seed)
    if key not in _WEIGHTS:
        rng = np.random.default_rng(1000 * seed + n + 7 * k + (layout == 'NT'))
        rows, cols = (n, k) if layout == 'NT' else (k, n)
        b = (rng.standard_normal([rows, cols]) / np.sqrt(k)).astype(np.float32)
        buf = np.full([rows + 1, cols + 8], np.nan, dtype=np.float32)
        buf[:rows, :cols] = b
        hbuf = np.full([rows + 1, cols + 8], np.nan, dtype=np.float16)
        hbuf[:rows, :cols] = b.astype(np.float16)
        _WEIGHTS[key] = (b, _rounded(b), D.from_host(buf), D.bytes_from_host(hbuf), cols + 8)
    return _WEIGHTS[key]


class Call:
    """One npm_sgemm_skinny_w16 call (``w16`` False: npm_sgemm_skinny on the fp32 originals) with every output in a
    sentinel-filled buffer and every input in a NaN-padded one."""

    def __init__(self, layout, a, n, k, epilogue=0, alpha=1.0, wide=True, seed=0, w16=True):
        from np_modeling_amd import _C, device as D
        self.layout, self.m, self.n, self.k, self.epilogue, self.alpha, self.w16 = layout, a.shape[0], n, k, epilogue, alpha, w16
        m = self.m
        self.a = a
        self.b32, self.b, self.b32_dev, self.b16_dev, ldb = _weights(layout, n, k, seed)
        pad = 4 if wide else 0
        lda, self.ldc, ldr, self.ldaux = k + pad, n + 2 * pad, n + 3 * pad, n + pad
        abuf = np.full([m + 2, lda], np.nan, dtype=np.float32)               # NaN past row M and past column K
        abuf[:m, :k] = a
        self.a_dev = D.from_host(abuf)
        rng = np.random.default_rng(m + n + k + epilogue)
        self.bias = rng.standard_normal([n]).astype(np.float32)
        self.residual = rng.standard_normal([m, n]).astype(np.float32)
        self.bias_dev = D.from_host(self.bias)
        rbuf = np.full([m, ldr], np.nan, dtype=np.float32)
        rbuf[:, :n] = self.residual
        self.res_dev = D.from_host(rbuf)
        self.rows = m + 2                                                     # two rows behind the result stay sentinels
        self.c_dev = D.full([2 * GUARD + self.rows * self.ldc], SENTINEL)
        self.aux_dev = D.full([2 * GUARD + self.rows * self.ldaux], SENTINEL)
        g = self.g = _C.npm_gemm()
        g.trans_a, g.trans_b, g.m, g.n, g.k, g.batch0, g.batch1 = 0, int(layout == 'NT'), m, n, k, 1, 1
        g.a, g.lda, g.b, g.ldb = self.a_dev.ptr, lda, (self.b16_dev if w16 else self.b32_dev).ptr, ldb
        g.c, g.ldc = self.c_dev.ptr + 4 * GUARD, self.ldc
        g.alpha, g.epilogue = alpha, epilogue
        if epilogue & SC.EPI_BIAS:
            g.bias = self.bias_dev.ptr
        if epilogue & SC.EPI_RESIDUAL:
            g.residual, g.ldr = self.res_dev.ptr, ldr
        if epilogue & SC.EPI_RELU_SAVE:
            g.aux, g.ldaux = self.aux_dev.ptr + 4 * GUARD, self.ldaux

    def _guarded(self, dev, ld, written):
        """The [m, n] result out of a buffer in which everything else still holds the sentinel, bit for bit."""
        host = dev.numpy()
        body = host[GUARD:GUARD + self.rows * ld].reshape(self.rows, ld)
        out = body[:self.m, :self.n].copy()
        if written:
            body[:self.m, :self.n] = SENTINEL
        assert (host.view(np.uint32) == np.float32(SENTINEL).view(np.uint32)).all(), 'a store outside the result'
        return out

    def run(self, expect=0):
        from np_modeling_amd import _C
        lib = _C.lib()
        name = 'npm_sgemm_skinny_w16' if self.w16 else 'npm_sgemm_skinny'
        says = getattr(lib, name + '_supported')(C.byref(self.g))
        rc = getattr(lib, name)(C.byref(self.g))
        assert says == int(rc == 0), (says, rc)                               # the predicate agrees with the entry point
        if expect:
            assert rc == expect, (rc, lib.npm_last_error())
            self._guarded(self.c_dev, self.ldc, False)
            self._guarded(self.aux_dev, self.ldaux, False)
            return None
        _C.check(rc, name)
        self.kernel = _C.last_skinny_kernel()
        c = self._guarded(self.c_dev, self.ldc, True)
        aux = self._guarded(self.aux_dev, self.ldaux, bool(self.epilogue & SC.EPI_RELU_SAVE))
        return c, (aux if self.epilogue & SC.EPI_RELU_SAVE else None)

    def check(self, c, aux, what):
        """Against float64 on the weights the call read: the rounded ones for w16."""
        want, want_pre = SC.reference(self.a, self.b if self.w16 else self.b32, self.layout, self.alpha, self.epilogue, self.bias,
                                      self.residual)
        pairs = [('C', c, want)] + ([('aux', aux, want_pre)] if want_pre is not None else [])
        worst = 0.0
        for name, got, ref in pairs:
            assert np.isfinite(got).all(), f'{what} {name}: not finite'
            scale = np.abs(ref).max()
            frac = float((np.abs(got.astype(np.float64) - ref) / (SC.TOL * (np.abs(ref) + scale) + 1e-30)).max())
            worst = max(worst, frac)
            print(f'{what} {name}: {frac:.3f} of {SC.TOL:.0e} (|ref| + max |ref|)  [{self.kernel}]')
            assert_close(got, ref, tol=SC.TOL, what=f'{what} {name}')
        return worst


def _a(m, k, seed, uniform=False):
    rng = np.random.default_rng(seed)
    return (rng.random([m, k]) if uniform else rng.standard_normal([m, k])).astype(np.float32)


def _same_bits(x, y):
    return x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))


# ---- 1. conversions --------------------------------------------------------------------------------------------------------------
def _special_floats():
    """What the rounding has to get right, as float32: normals, +-0, ties at the half spacing (to even, up and down), values whose
    halves are subnormal, values that flush to 0 (2^-25 is the tie between 0 and the smallest subnormal: to even, 0), the largest
    finite half, the last value that rounds to it, the first that becomes inf, infinities and NaN."""
    f = np.float32
    ties = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 2.0 ** -11 - 2.0 ** -23, 2048.0 + 1.0, 2048.0 + 3.0,
            -(1 + 2.0 ** -11), 0.1, -0.1, 1 / 3, 1000.7, 3.14159265]
    sub = [2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -15, 3.0 * 2.0 ** -24, 2.5 * 2.0 ** -24, 1.5 * 2.0 ** -24, 2.0 ** -24, 6.1e-5, 3e-6, -3e-6,
           2.0 ** -25 * (1 + 2.0 ** -20)]
    flush = [2.0 ** -25, -2.0 ** -25, 2.0 ** -26, 1e-10, -1e-30, 1e-45, 0.0, -0.0]
    top = [65504.0, 65519.99, 65520.0, -65519.99, -65520.0, 65536.0, 1e9, 3.4e38, np.inf, -np.inf, np.nan]
    return np.array(ties + sub + flush + top, dtype=f)


def _half_guarded(rows, pitch):
    from np_modeling_amd import device as D
    return D.bytes_from_host(np.full([GUARD + rows * pitch + GUARD], HALF_SENTINEL, dtype=np.uint16))


def test_cvt_f32_f16_is_bitwise_numpy_astype(npm):
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    special = _special_floats()
    rng = np.random.default_rng(0)
    # (rows, cols, source pitch, destination pitch, byte offset of the destination): the 16-byte path, then the element path (odd
    # width; odd pitches; a destination that is only 2-byte aligned)
    for rows, cols, sp, dp, shift in ((9, 40, 44, 48, 0), (9, 37, 41, 43, 0), (9, 40, 44, 48, 1), (1, 8, 8, 8, 0)):
        src = (rng.standard_normal([rows, sp]) * 10.0 ** rng.integers(-9, 6, [rows, sp])).astype(np.float32)
        flat = src[:, :cols].reshape(-1)
        take = min(special.size, flat.size)
        flat[:take] = special[:take]
        src[:, :cols] = flat.reshape(rows, cols)
        src[:, cols:] = np.nan                                                # the pitch padding is not read into anything
        src_dev = D.from_host(src)
        dst = _half_guarded(rows, dp)
        first = GUARD + shift
        assert lib.npm_cvt_f32_f16(src_dev.ptr, sp, dst.ptr + 2 * first, dp, rows, cols) == 0, lib.npm_last_error()
        host = dst.numpy().view(np.uint16).copy()
        body = host[first:first + rows * dp].reshape(rows, dp)
        got = body[:, :cols].copy()
        body[:, :cols] = HALF_SENTINEL
        assert (host == HALF_SENTINEL).all(), 'a store outside the destination'
        with np.errstate(over='ignore'):
            want = src[:, :cols].astype(np.float16)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got.view(np.float16)), nan) and (take < special.size or nan.sum() == 1)
        same = got == want.view(np.uint16)
        assert same[~nan].all(), (rows, cols, src[:, :cols][~same & ~nan][:8], got[~same & ~nan][:8])
        if take == special.size:
            assert np.isinf(got.view(np.float16)).sum() >= 7 and (got.view(np.float16) == np.float16(65504)).sum() >= 2
    assert lib.npm_cvt_f32_f16(None, 0, None, 0, 0, 0) == 0 and lib.npm_cvt_f32_f16(None, 8, None, 8, 0, 8) == 0
    assert lib.npm_cvt_f32_f16(src_dev.ptr, 4, dst.ptr, 8, 1, 8) == BAD_ARGUMENT        # a pitch below the width


def test_cvt_f16_f32_is_exact_on_every_finite_half(npm):
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    patterns = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    patterns = patterns[(patterns & 0x7C00) != 0x7C00]
    assert patterns.size == 63488
    want = patterns.view(np.float16).astype(np.float32)
    for rows, cols, sp, dp, shift in ((248, 256, 264, 260, 0), (1, 63487, 63488, 63487, 1)):
        src = np.full([rows, sp], 0x7E00, dtype=np.uint16)                    # NaN in the pitch padding
        take = patterns[shift:shift + rows * cols].reshape(rows, cols)
        src[:, :cols] = take
        src_dev = D.bytes_from_host(np.concatenate([np.zeros(shift, np.uint16), src.reshape(-1)]))
        out = D.full([2 * GUARD + rows * dp], SENTINEL)
        assert lib.npm_cvt_f16_f32(src_dev.ptr + 2 * shift, sp, out.ptr + 4 * GUARD, dp, rows, cols) == 0, lib.npm_last_error()
        host = out.numpy()
        body = host[GUARD:GUARD + rows * dp].reshape(rows, dp)
        got = body[:, :cols].copy()
        body[:, :cols] = SENTINEL
        assert (host.view(np.uint32) == np.float32(SENTINEL).view(np.uint32)).all(), 'a store outside the destination'
        assert _same_bits(got, want[shift:shift + rows * cols].reshape(rows, cols))
    assert lib.npm_cvt_f16_f32(None, 0, None, 0, 0, 0) == 0


# ---- 2. the kernel against float64 on the rounded weights -------------------------------------------------------------------------
@pytest.mark.parametrize('n,k', SHAPES)
@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_kernel_against_float64_on_the_rounded_weights(npm, layout, n, k):
    """Every M x every epilogue x every alpha; the data distribution and the pitches rotate."""
    from np_modeling_amd import _C
    splits = _C.lib().npm_sgemm_skinny_splits(n, k, int(layout == 'NT'))
    worst = 0.0
    for i, m in enumerate(ROWS):
        for j, epilogue in enumerate(SC.EPILOGUES):
            for alpha in ALPHAS:
                call = Call(layout, _a(m, k, seed=m + k + j, uniform=(i + j) % 4 == 3), n, k, epilogue, alpha, wide=(i + j) % 2 == 0)
                c, aux = call.run()
                assert call.kernel == f'sgemm_skinny_kernel {layout} M={m} N={n} K={k} rb={(m + 15) // 16} splits={splits} nt=0 w=f16'
                worst = max(worst, call.check(c, aux, f'{layout} M={m} N={n} K={k} epi={epilogue} alpha={alpha}'))
    print(f'{layout} N={n} K={k}: worst {worst:.3f} of the bound')


@pytest.mark.parametrize('n,k', SHAPES)
@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_forced_splits_pass_the_same_bound(npm, layout, n, k):
    for forced in (1, 7):
        _tune(SPLITS_KNOB, forced)
        for m, epilogue in ((5, SC.EPI_BIAS | SC.EPI_RESIDUAL), (40, SC.EPI_BIAS | SC.EPI_RELU_SAVE), (64, 0)):
            call = Call(layout, _a(m, k, seed=forced + m, uniform=forced == 1), n, k, epilogue, 1.25)
            c, aux = call.run()
            assert f' splits={forced} ' in call.kernel and call.kernel.endswith(' w=f16')
            call.check(c, aux, f'{layout} M={m} N={n} K={k} forced splits {forced}')


# ---- 3. bitwise properties -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_same_call_twice_and_either_load_hint_are_bitwise_equal(npm, layout):
    for n, k in SHAPES:
        for m, epilogue in ((3, SC.EPI_BIAS), (64, SC.EPI_BIAS | SC.EPI_RELU_SAVE)):
            call = Call(layout, _a(m, k, seed=9), n, k, epilogue)
            first = call.run()
            again = call.run()
            assert call.kernel.endswith('nt=0 w=f16')
            _tune(NT_KNOB, 1)
            hinted = call.run()
            assert call.kernel.endswith('nt=1 w=f16')
            _tune(NT_KNOB, 2)
            plain = call.run()
            assert call.kernel.endswith('nt=0 w=f16')
            _tune(NT_KNOB, 0)
            for other in (again, hinted, plain):
                assert _same_bits(first[0], other[0]) and (first[1] is None or _same_bits(first[1], other[1]))


@pytest.mark.parametrize('forced', [0, 7])
@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_a_row_does_not_depend_on_m_or_on_its_position(npm, layout, forced):
    """Row r of an M-row call is bitwise the M = 1 call on that row alone: first, middle and last row."""
    _tune(SPLITS_KNOB, forced)
    for n, k in SHAPES:
        for m in (2, 17, 64):
            a = _a(m, k, seed=m + n)
            for epilogue in (SC.EPI_BIAS | SC.EPI_RESIDUAL, SC.EPI_BIAS | SC.EPI_RELU_SAVE):
                whole = Call(layout, a, n, k, epilogue, 0.5)
                c, aux = whole.run()
                for r in sorted({0, m // 2, m - 1}):
                    one = Call(layout, a[r:r + 1], n, k, epilogue, 0.5)
                    one.bias_dev.set(whole.bias)
                    one.res_dev.set(np.pad(whole.residual[r:r + 1], ((0, 0), (0, one.res_dev.shape[1] - n))))
                    c1, aux1 = one.run()
                    assert _same_bits(c1[0], c[r]), (layout, forced, n, k, m, epilogue, r)
                    assert aux is None or _same_bits(aux1[0], aux[r])


@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_the_kernel_string_is_the_fp32_string_plus_the_suffix(npm, layout):
    from np_modeling_amd import _C
    for n, k in SHAPES:
        for m in (1, 33):
            a = _a(m, k, seed=4)
            half = Call(layout, a, n, k, SC.EPI_BIAS)
            half.run()
            full = Call(layout, a, n, k, SC.EPI_BIAS, w16=False)
            full.run()
            assert half.kernel == full.kernel + ' w=f16' and ' w=' not in full.kernel
            assert _C.last_skinny_kernel() == full.kernel                     # npm_sgemm_skinny afterwards reports no suffix


@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_w16_is_bitwise_the_fp32_kernel_on_the_rounded_weights(npm, layout):
    """What include/npm_hip.h states for the shipped load mapping (the lane-to-k mapping of the fp32 instance is kept)."""
    from np_modeling_amd import device as D
    for n, k in SHAPES:
        _, rounded, _, _, ldb = _weights(layout, n, k)
        buf = np.full([rounded.shape[0] + 1, ldb], np.nan, dtype=np.float32)
        buf[:rounded.shape[0], :rounded.shape[1]] = rounded
        rounded_dev = D.from_host(buf)
        for m, epilogue in ((1, 0), (17, SC.EPI_BIAS | SC.EPI_RESIDUAL), (33, SC.EPI_BIAS), (64, SC.EPI_BIAS | SC.EPI_RELU_SAVE)):
            a = _a(m, k, seed=m)
            half = Call(layout, a, n, k, epilogue, 0.37)
            full = Call(layout, a, n, k, epilogue, 0.37, w16=False)
            full.g.b = rounded_dev.ptr
            (c16, aux16), (c32, aux32) = half.run(), full.run()
            assert _same_bits(c16, c32) and (aux16 is None or _same_bits(aux16, aux32)), (layout, n, k, m)


# ---- 4. nothing outside the operands ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_nothing_outside_the_operands_is_read(npm, layout):
    """A's rows past M and columns past K, B's rows past N (NT) and columns past N or K inside its pitch hold NaN in every call of
    this file; here the same product with zero padding gives the same bits, and a NaN INSIDE an operand reaches exactly its row
    (A) or its column (B)."""
    from np_modeling_amd import device as D
    for n, k in SHAPES:
        for m in ((1, 15, 16, 17, 33, 64) if k < 1024 else (1, 17, 64)):
            a = _a(m, k, seed=m)
            call = Call(layout, a, n, k, SC.EPI_BIAS)
            c, _ = call.run()
            clean = Call(layout, a, n, k, SC.EPI_BIAS)
            abuf = np.zeros(clean.a_dev.shape, dtype=np.float32)
            abuf[:m, :k] = a
            clean.a_dev.set(abuf)
            b32, _, _, _, ldb = _weights(layout, n, k)
            bbuf = np.zeros([b32.shape[0] + 1, ldb], dtype=np.float16)
            bbuf[:b32.shape[0], :b32.shape[1]] = b32.astype(np.float16)
            clean.b16_dev = D.bytes_from_host(bbuf)
            clean.g.b = clean.b16_dev.ptr
            c2, _ = clean.run()
            assert _same_bits(c, c2)
            abuf[m - 1, k - 1] = np.nan
            clean.a_dev.set(abuf)
            c3, _ = clean.run()
            assert np.isnan(c3[m - 1]).all() and np.isfinite(c3[:m - 1]).all()
            abuf[m - 1, k - 1] = a[m - 1, k - 1]
            clean.a_dev.set(abuf)
            col = n - 1                                                       # a NaN weight of the last output column, at the last k
            bbuf[(col, k - 1) if layout == 'NT' else (k - 1, col)] = np.nan
            clean.b16_dev = D.bytes_from_host(bbuf)
            clean.g.b = clean.b16_dev.ptr
            c4, _ = clean.run()
            assert np.isnan(c4[:, col]).all() and np.isfinite(np.delete(c4, col, axis=1)).all()
            assert _same_bits(np.delete(c4, col, axis=1), np.delete(c, col, axis=1))


# ---- 5. distance from the fp32 weights -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,k', SHAPES)
@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_distance_from_the_product_on_the_fp32_weights(npm, layout, n, k):
    for m in (1, 17, 64):
        a = _a(m, k, seed=2 * m + 1)
        half = Call(layout, a, n, k)
        y16, _ = half.run()
        full = Call(layout, a, n, k, w16=False)
        y32, _ = full.run()
        full.check(y32, None, f'{layout} M={m} N={n} K={k} fp32 weights')
        a64, w64 = np.abs(a.astype(np.float64)), np.abs(half.b32.astype(np.float64))
        mass = a64 @ (w64.T if layout == 'NT' else w64)                        # sum_k |a_k w_k|
        y32 = y32.astype(np.float64)
        bound = 2.0 ** -11 * mass + 2.0 ** -25 * a64.sum(axis=1, keepdims=True) + SC.TOL * (np.abs(y32) + np.abs(y32).max())
        frac = float((np.abs(y16.astype(np.float64) - y32) / bound).max())
        print(f'{layout} M={m} N={n} K={k}: |y16 - y32| uses {frac:.3f} of its bound; max |y16 - y32| = {np.abs(y16 - y32).max():.3e}, '
              f'max |y32| = {np.abs(y32).max():.3e}')
        assert frac <= 1.0 and not _same_bits(y16, y32.astype(np.float32))


# ---- 6. unsupported arguments ----------------------------------------------------------------------------------------------------
def test_unsupported_arguments_write_nothing_and_the_predicate_agrees(npm):
    from np_modeling_amd import _C, device as D
    spare = D.zeros([64])

    def refused(change, m=8):
        call = Call('NT', _a(m, 32, seed=1), 48, 32, SC.EPI_BIAS)
        assert call.g.ldb == 40
        change(call.g)
        assert call.run(expect=UNSUPPORTED) is None
        assert b'npm_sgemm_skinny_w16' in _C.lib().npm_last_error()

    refused(lambda g: setattr(g, 'ldb', 36))                              # a multiple of 4 halves is not enough
    refused(lambda g: setattr(g, 'ldb', 44))
    refused(lambda g: setattr(g, 'b', g.b + 8))                           # b on an 8-byte boundary
    refused(lambda g: setattr(g, 'b', g.b + 2))
    refused(lambda g: setattr(g, 'ldb', 24))                              # below the width
    refused(lambda g: setattr(g, 'trans_a', 1))                           # what tests/test_gpu_skinny.py lists
    refused(lambda g: setattr(g, 'batch0', 2))
    refused(lambda g: setattr(g, 'batch1', 3))
    refused(lambda g: None, m=65)
    refused(lambda g: setattr(g, 'bsum', spare.ptr))
    refused(lambda g: setattr(g, 'colsum', spare.ptr))
    refused(lambda g: setattr(g, 'asum', spare.ptr))
    refused(lambda g: setattr(g, 'rowdot', spare.ptr))
    refused(lambda g: setattr(g, 'split_k', 2))
    refused(lambda g: setattr(g, 'a', g.a + 4))
    refused(lambda g: setattr(g, 'c', g.c + 8))
    refused(lambda g: setattr(g, 'bias', g.bias + 4))
    refused(lambda g: setattr(g, 'lda', 34))
    refused(lambda g: setattr(g, 'ldc', 44))
    refused(lambda g: setattr(g, 'n', 40))
    refused(lambda g: setattr(g, 'k', 24))
    refused(lambda g: setattr(g, 'epilogue', 8))
    refused(lambda g: setattr(g, 'epilogue', 32))
    refused(lambda g: setattr(g, 'epilogue', SC.EPI_RELU | SC.EPI_RELU_SAVE))
    ok = Call('NT', _a(8, 32, seed=1), 48, 32, SC.EPI_BIAS)
    c, _ = ok.run()
    ok.check(c, None, 'the unchanged call')
    assert _C.lib().npm_sgemm_skinny_w16(None) == BAD_ARGUMENT and _C.lib().npm_sgemm_skinny_w16_supported(None) == 0


# ---- 7. layers -------------------------------------------------------------------------------------------------------------------
def _layer_close(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    frac = float((np.abs(got - want) / (tol * (np.abs(want) + max(np.abs(want).max(), 1.0)))).max())
    print(f'{what}: {frac:.3f} of {tol:.1e} (|ref| + max |ref|)')
    assert frac <= 1.0, f'{what}: {frac:.3g} of the bound {tol:.3g}'


def _timed(npm, run):
    with npm.device.KernelTimer() as timer:
        out = run()
    return out, set(timer.summary())


def _no_w16(names):
    return not any('w16' in n or n.startswith('cvt_') for n in names)


@pytest.mark.parametrize('kind', ['contiguous', 'ragged', 'paged'])
@pytest.mark.parametrize('heads,kv_heads,f', [(8, 8, 1024), (8, 2, 1024), (4, 2, 64)])
def test_attention_with_a_cache_and_half_weights(npm, heads, kv_heads, f, kind):
    att, _ = DC.make_mha(npm, f, heads, kv_heads, seed=heads + f, batch=3)
    twin, _ = DC.make_mha(npm, f, heads, kv_heads, seed=heads + f, batch=3)
    for name in ('_wq', '_wk', '_wv', '_wo'):
        getattr(twin, name).set(_rounded(np.asarray(getattr(twin, name))))
    p = {n: np.asarray(getattr(twin, '_' + n)).astype(np.float64) for n in DC.ATT}
    if kind == 'contiguous':
        schedule = [np.array(n) for n in ([5, 5, 5], [1, 1, 1], [1, 1, 1], [3, 3, 3], [1, 1, 1])]
    else:
        schedule = [np.array(n) for n in ([5, 2, 9], [1, 1, 1], [1, 0, 1], [3, 1, 2], [1, 1, 1])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(f)
    x_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    want = VR.layer_alone(p, x_rows, schedule)
    paged = dict(page_size=16) if kind == 'paged' else {}

    def run(layer, **kwargs):
        cache = layer.make_cache(3, int(total.max()) + 2, **paged)
        outs = []
        for x, n in VR.padded_calls(x_rows, schedule):
            outs.append(np.asarray(layer(x, cache=cache, new_lengths=None if kind == 'contiguous' else n, **kwargs)))
        return VR.collect(outs, schedule, 3)

    hw, made = _timed(npm, att.half_weights)
    assert made == {'cvt_f32_f16'}
    got, names = _timed(npm, lambda: run(att, weights=hw))
    assert 'sgemm_skinny_w16_NT' in names and not names & {'sgemm_NT', 'sgemm_skinny_NT', 'cvt_f16_f32'}, names
    twin_out, twin_names = _timed(npm, lambda: run(twin))
    assert _no_w16(twin_names) and 'sgemm_skinny_NT' in twin_names
    plain, plain_names = _timed(npm, lambda: run(att))                      # the layer itself without the keyword: fp32 weights
    assert _no_w16(plain_names)
    for b in range(3):
        _layer_close(got[b], want[b], SC.LAYER_TOL, f'{kind} H{heads}/{kv_heads} F{f} sequence {b} half weights vs float64 on the rounded')
        _layer_close(got[b], twin_out[b], 2 * SC.LAYER_TOL, f'{kind} H{heads}/{kv_heads} F{f} sequence {b} half weights vs twin')
        assert not np.array_equal(got[b], plain[b])


def _round_six(dec):
    for path, attr in SIX:
        arr = getattr(DC.sub(dec, path), attr)
        arr.set(_rounded(np.asarray(arr)))


def _decode_chunks(dec, q, kv, sizes, capacity, **kwargs):
    state = dec.start_decoding(kv, capacity, **kwargs)
    outs = [np.asarray(dec.decode(np.ascontiguousarray(piece), state)) for piece in DC.split(q, sizes)]
    assert state.position == sum(sizes)
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('kv_heads', [None, 2])
def test_decoder_decode_with_half_weights(npm, norm_first, kv_heads):
    from np_modeling_amd import _C
    D = npm.device
    f, s = 256, 23
    dec, _ = DC.make_decoder(npm, f, 4, kv_heads, 384, norm_first, True, seed=11, batch=3, seq_kv=23)
    twin, _ = DC.make_decoder(npm, f, 4, kv_heads, 384, norm_first, True, seed=11, batch=3, seq_kv=23)
    _round_six(twin)
    p = DC.decoder_params(twin)
    rng = np.random.default_rng(12)
    q, kv = rng.standard_normal([3, s, f]).astype(np.float32), rng.standard_normal([3, 23, f]).astype(np.float32)
    want, _ = DR.decoder_fwd(p, q.astype(np.float64), kv.astype(np.float64), norm_first, mask=DR.causal_mask(s))
    for sizes in DC.chunkings(21):                                        # [21] is M = 63: the largest chunk the w16 kernel takes here
        got, names = _timed(npm, lambda: _decode_chunks(dec, q[:, :21], kv, sizes, capacity=s + 3, weights='f16'))
        assert {'cvt_f32_f16', 'sgemm_skinny_w16_NT', 'sgemm_skinny_w16_NN'} <= names and 'cvt_f16_f32' not in names, names
        assert not names & {'sgemm_skinny_NT', 'sgemm_skinny_NN', 'sgemm_NN'}, names      # sgemm_NT: the memory projection, fp32
        twin_out, twin_names = _timed(npm, lambda: _decode_chunks(twin, q[:, :21], kv, sizes, capacity=s + 3))
        assert _no_w16(twin_names)
        _layer_close(got, want[:, :21], SC.LAYER_TOL, f'decode chunks {sizes[:4]} half weights vs float64 on the rounded')
        _layer_close(got, twin_out, 2 * SC.LAYER_TOL, f'decode chunks {sizes[:4]} half weights vs twin')
    # a chunk of B T = 66 > 64 rows converts the halves back and runs npm_sgemm on them; the steps behind it run the w16 kernel
    state = dec.start_decoding(kv, s + 3, weights='f16')
    twin_state = twin.start_decoding(kv, s + 3)
    big, names = _timed(npm, lambda: np.asarray(dec.decode(np.ascontiguousarray(q[:, :22]), state)))
    assert {'cvt_f16_f32', 'sgemm_NT', 'sgemm_NN'} <= names and not any('skinny' in n for n in names), names
    step, step_names = _timed(npm, lambda: np.asarray(dec.decode(np.ascontiguousarray(q[:, 22:]), state)))
    assert {'sgemm_skinny_w16_NT', 'sgemm_skinny_w16_NN'} <= step_names and not step_names & {'cvt_f16_f32', 'sgemm_NT', 'sgemm_NN'}, step_names
    assert _C.last_skinny_kernel().startswith('sgemm_skinny_kernel NN M=3 N=256 K=384 rb=1 ') and _C.last_skinny_kernel().endswith(' w=f16')
    got = np.concatenate([big, step], axis=1)
    twin_out = np.concatenate([np.asarray(twin.decode(np.ascontiguousarray(x), twin_state)) for x in (q[:, :22], q[:, 22:])], axis=1)
    _layer_close(got, want, SC.LAYER_TOL, 'decode chunks [22, 1] half weights vs float64 on the rounded')
    _layer_close(got, twin_out, 2 * SC.LAYER_TOL, 'decode chunks [22, 1] half weights vs twin')
    # another math mode: no w16 kernel, the halves converted back; without the keyword neither a w16 nor a cvt name
    state = dec.start_decoding(kv, s + 3, weights='f16')
    before = _C.last_skinny_kernel()
    npm.set_math('bf16x3')
    try:
        _, names = _timed(npm, lambda: dec.decode(q[:, :1], state))
    finally:
        npm.set_math('f32')
    assert not any('skinny' in n for n in names) and {'cvt_f16_f32', 'sgemm_NT', 'sgemm_NN'} <= names and _C.last_skinny_kernel() == before
    for kwargs in ({}, dict(weights=None)):
        _, names = _timed(npm, lambda: _decode_chunks(dec, q[:, :4], kv, [3, 1], capacity=s + 3, **kwargs))
        assert _no_w16(names) and {'sgemm_skinny_NT', 'sgemm_skinny_NN'} <= names, names


@pytest.mark.parametrize('cache_dtype,page_size', [('f16', None), ('f32', 16)])
def test_half_weights_beside_an_fp16_cache_a_paged_cache_and_rope(npm, cache_dtype, page_size):
    """None of the caches looks at the weights: the same twin relation with an fp16 cache, a paged cache and rotary embeddings."""
    f, s = 256, 9
    kwargs = dict(cache_dtype=cache_dtype, **({} if page_size is None else dict(page_size=page_size)))

    def make():
        np.random.seed(21)
        dec = npm.layers.TransformerDecoder(num_heads=4, hidden_units=384, norm_first=True, num_kv_heads=2, causal=True, rope_base=10000.0)
        dec(np.zeros([2, 2, f], dtype=np.float32), np.zeros([2, 7, f], dtype=np.float32))
        for path, attr in SIX + (('_cross_attention', '_wk'), ('_cross_attention', '_wv')):
            arr = getattr(DC.sub(dec, path), attr)
            arr.set(np.asarray(arr) * np.float32(2.0 / np.sqrt(f)))
        return dec

    dec, twin = make(), make()
    _round_six(twin)
    rng = np.random.default_rng(22)
    q, kv = rng.standard_normal([2, s, f]).astype(np.float32), rng.standard_normal([2, 7, f]).astype(np.float32)
    got, names = _timed(npm, lambda: _decode_chunks(dec, q, kv, [5, 1, 3], capacity=16, weights='f16', **kwargs))
    assert {'sgemm_skinny_w16_NT', 'sgemm_skinny_w16_NN'} <= names and 'cvt_f16_f32' not in names
    twin_out = _decode_chunks(twin, q, kv, [5, 1, 3], capacity=16, **kwargs)
    # every product here has M <= 64 rows, so each is the w16 kernel against the fp32 skinny kernel on the rounded values: the same
    # bits (include/npm_hip.h), hence the same rows in either cache and the same output
    assert np.array_equal(got.view(np.uint32), twin_out.view(np.uint32))
