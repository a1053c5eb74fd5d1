"""MI355X: the skinny-M GEMM (npm_sgemm_skinny, csrc/npm_skinny.hip) against float64 NumPy, and the layers that use it.

The parity bound is 2e-6 in conftest.assert_close's metric, the project's bound for single GEMM kernels (tests/test_gpu_gemm.py):
emulating fp32 fma chains at K = 4096, M 16 - 64 on N(0, 1) and U(0, 1) data, ONE sequential chain per element reaches 1.3e-6 -
1.8e-6 of that metric, four interleaved chains <= 6.2e-7, sixteen <= 2.5e-7; the kernel adds at least four partial sums per
element (the four waves of a block, times the splits), so the bound has a threefold margin and a case that needs more is a bug.
Layers: LAYER_TOL = 1e-5 against tests/decode_reference.py and 2 LAYER_TOL between the two routes, tests/test_gpu_decode.py's
bounds for decode against forward.  Every test prints the fraction of its bound it used before it asserts.
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
SPLITS_KNOB, NT_KNOB = 22, 23
MAX_SPLITS = 64
UNSUPPORTED = 10003


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


_WEIGHTS = {}


def _weights(layout, n, k, seed=0):
    """B of one (layout, N, K) on the device, once per process: rows 8 floats wider than the matrix and, for NT, one more row
    than N; everything outside the matrix is NaN.  Returns (host matrix as stored, device array, ldb)."""
    from np_modeling_amd import device as D
    key = (layout, n, k, seed)
    if key not in _WEIGHTS:
        rng = np.random.default_rng(1000 * seed + n + 7 * k + (layout == 'NT'))
        rows, cols = (n, k) if layout == 'NT' else (k, n)
        b = (rng.standard_normal([rows, cols]) / np.sqrt(k)).astype(np.float32)
        buf = np.full([rows + 1, cols + 8], np.nan, dtype=np.float32)
        buf[:rows, :cols] = b
        _WEIGHTS[key] = (b, D.from_host(buf), cols + 8)
    return _WEIGHTS[key]


class Call:
    """One npm_sgemm_skinny call with every output in a sentinel-filled buffer and every input in a NaN-padded one."""

    def __init__(self, layout, a, n, k, epilogue=0, alpha=1.0, wide=True, seed=0, poison_rows=2):
        from np_modeling_amd import _C, device as D
        self.layout, self.m, self.n, self.k, self.epilogue, self.alpha = layout, a.shape[0], n, k, epilogue, alpha
        m = self.m
        self.a = a
        self.b, self.b_dev, ldb = _weights(layout, n, k, seed)
        pad = 4 if wide else 0
        lda, self.ldc, ldr, self.ldaux = k + pad, n + 2 * pad, n + 3 * pad, n + pad
        abuf = np.full([m + poison_rows, lda], np.nan, dtype=np.float32)      # NaN past row M and past column K
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
        g.a, g.lda, g.b, g.ldb = self.a_dev.ptr, lda, self.b_dev.ptr, ldb
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
        says = lib.npm_sgemm_skinny_supported(C.byref(self.g))
        rc = lib.npm_sgemm_skinny(C.byref(self.g))
        assert says == int(rc == 0), (says, rc)                               # the predicate agrees with the entry point
        if expect:
            assert rc == expect, (rc, lib.npm_last_error())
            self._guarded(self.c_dev, self.ldc, False)
            self._guarded(self.aux_dev, self.ldaux, False)
            return None
        _C.check(rc, 'npm_sgemm_skinny')
        self.kernel = _C.last_skinny_kernel()
        c = self._guarded(self.c_dev, self.ldc, True)
        aux = self._guarded(self.aux_dev, self.ldaux, bool(self.epilogue & SC.EPI_RELU_SAVE))
        return c, (aux if self.epilogue & SC.EPI_RELU_SAVE else None)

    def check(self, c, aux, what):
        want, want_pre = SC.reference(self.a, self.b, self.layout, self.alpha, self.epilogue, self.bias, self.residual)
        pairs = [('C', c, want)] + ([('aux', aux, want_pre)] if want_pre is not None else [])
        for name, got, ref in pairs:
            assert np.isfinite(got).all(), f'{what} {name}: not finite'
            scale = np.abs(ref).max()
            frac = float((np.abs(got.astype(np.float64) - ref) / (SC.TOL * (np.abs(ref) + scale) + 1e-30)).max())
            print(f'{what} {name}: {frac:.3f} of {SC.TOL:.0e} (|ref| + max |ref|)  [{self.kernel}]')
            assert_close(got, ref, tol=SC.TOL, what=f'{what} {name}')


def _a(m, k, seed, uniform=False):
    rng = np.random.default_rng(seed)
    return (rng.random([m, k]) if uniform else rng.standard_normal([m, k])).astype(np.float32)


def test_case_grid_is_the_one_the_kernel_was_specified_on():
    assert SC.ROWS == (1, 2, 3, 15, 16, 17, 31, 32, 33, 48, 63, 64) and SC.LAYOUTS == ('NT', 'NN')
    for shape in ((16, 16), (48, 32), (272, 528), (1024, 1024), (1536, 1024), (3072, 1024), (4096, 1024), (1024, 4096)):
        assert shape in SC.SHAPES
    assert {1, 3, 17, 5} <= set(SC.EPILOGUES)


@pytest.mark.parametrize('n,k', SC.SHAPES)
@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_kernel_against_float64(npm, layout, n, k):
    """Every M of the grid; the epilogue, alpha, the data distribution and the pitches rotate with M so that every shape sees
    every epilogue (test_every_epilogue_at_every_row_block crosses them fully on three shapes)."""
    from np_modeling_amd import _C
    splits = _C.lib().npm_sgemm_skinny_splits(n, k, int(layout == 'NT'))
    for i, m in enumerate(SC.ROWS):
        epilogue = SC.EPILOGUES[(i + n // 16) % len(SC.EPILOGUES)]
        alpha = (1.0, 0.37, -1.5)[i % 3]
        call = Call(layout, _a(m, k, seed=m + k, uniform=i % 4 == 3), n, k, epilogue, alpha, wide=i % 2 == 0)
        c, aux = call.run()
        assert call.kernel == f'sgemm_skinny_kernel {layout} M={m} N={n} K={k} rb={(m + 15) // 16} splits={splits} nt=0'
        call.check(c, aux, f'{layout} M={m} N={n} K={k} epi={epilogue} alpha={alpha}')


@pytest.mark.parametrize('n,k', [(48, 32), (272, 528), (1024, 1024)])
@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_every_epilogue_at_every_row_block(npm, layout, n, k):
    for m in (1, 16, 17, 33, 64):
        for epilogue in SC.EPILOGUES:
            for alpha in (1.0, 0.73):
                call = Call(layout, _a(m, k, seed=3 * m + epilogue), n, k, epilogue, alpha)
                c, aux = call.run()
                call.check(c, aux, f'{layout} M={m} N={n} K={k} epi={epilogue} alpha={alpha}')


@pytest.mark.parametrize('n,k', [(48, 32), (272, 528), (1024, 4096), (4096, 1024)])
@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_forced_splits_pass_the_same_bound(npm, layout, n, k):
    for forced in (1, 2, 7, MAX_SPLITS, min(k // 16 + 3, MAX_SPLITS)):
        _tune(SPLITS_KNOB, forced)
        for m, epilogue in ((5, SC.EPI_BIAS | SC.EPI_RESIDUAL), (40, SC.EPI_BIAS | SC.EPI_RELU_SAVE)):
            call = Call(layout, _a(m, k, seed=forced + m, uniform=forced == 1), n, k, epilogue, 1.25)
            c, aux = call.run()
            assert f' splits={forced} ' in call.kernel
            call.check(c, aux, f'{layout} M={m} N={n} K={k} forced splits {forced}')
    from np_modeling_amd import _C
    assert _C.lib().npm_set_tuning(SPLITS_KNOB, MAX_SPLITS + 1) == 10002 and _C.lib().npm_set_tuning(NT_KNOB, 3) == 10002


@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_same_call_twice_and_either_load_policy_are_bitwise_equal(npm, layout):
    for n, k in ((272, 528), (4096, 1024)):
        for m, epilogue in ((3, SC.EPI_BIAS), (64, SC.EPI_BIAS | SC.EPI_RELU_SAVE)):
            call = Call(layout, _a(m, k, seed=9), n, k, epilogue)
            first = call.run()
            again = call.run()
            assert call.kernel.endswith('nt=0')
            _tune(NT_KNOB, 1)
            hinted = call.run()
            assert call.kernel.endswith('nt=1')
            _tune(NT_KNOB, 2)
            plain = call.run()
            assert call.kernel.endswith('nt=0')
            _tune(NT_KNOB, 0)
            for other in (again, hinted, plain):
                assert np.array_equal(first[0], other[0]) and (first[1] is None or np.array_equal(first[1], other[1]))


@pytest.mark.parametrize('forced', [0, 7])
@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_a_row_does_not_depend_on_m_or_on_its_position(npm, layout, forced):
    """Row r of an M-row call is bitwise the M = 1 call on that row alone: first, last and an interior row."""
    _tune(SPLITS_KNOB, forced)
    for n, k in ((272, 528), (1024, 1024)):
        for m in (2, 16, 17, 64):
            a = _a(m, k, seed=m + n)
            for epilogue in SC.EPILOGUES:
                whole = Call(layout, a, n, k, epilogue, 0.5)
                c, aux = whole.run()
                for r in sorted({0, m // 2, m - 1}):
                    one = Call(layout, a[r:r + 1], n, k, epilogue, 0.5)
                    one.bias_dev.set(whole.bias)
                    one.res_dev.set(np.pad(whole.residual[r:r + 1], ((0, 0), (0, one.res_dev.shape[1] - n))))
                    c1, aux1 = one.run()
                    assert np.array_equal(c1[0].view(np.uint32), c[r].view(np.uint32)), (layout, forced, n, k, m, epilogue, r)
                    assert aux is None or np.array_equal(aux1[0].view(np.uint32), aux[r].view(np.uint32))


@pytest.mark.parametrize('layout', SC.LAYOUTS)
def test_nothing_outside_the_operands_is_read(npm, layout):
    """A's rows past M and columns past K, B's rows past N (NT) and columns past N or K inside its pitch hold NaN in every call of
    this file; here the same product with finite padding gives the same bits, and a NaN INSIDE an operand does reach the result."""
    from np_modeling_amd import device as D
    for n, k in ((48, 32), (272, 528)):
        for m in (1, 15, 33):
            a = _a(m, k, seed=m)
            call = Call(layout, a, n, k, SC.EPI_BIAS)
            c, _ = call.run()
            clean = Call(layout, a, n, k, SC.EPI_BIAS)
            abuf = np.zeros(clean.a_dev.shape, dtype=np.float32)
            abuf[:m, :k] = a
            clean.a_dev.set(abuf)
            b, _, ldb = _weights(layout, n, k)
            bbuf = np.zeros([b.shape[0] + 1, ldb], dtype=np.float32)
            bbuf[:b.shape[0], :b.shape[1]] = b
            clean.b_dev = D.from_host(bbuf)
            clean.g.b = clean.b_dev.ptr
            c2, _ = clean.run()
            assert np.array_equal(c.view(np.uint32), c2.view(np.uint32))
            abuf[m - 1, k - 1] = np.nan
            clean.a_dev.set(abuf)
            c3, _ = clean.run()
            assert np.isnan(c3[m - 1]).all() and np.isfinite(c3[:m - 1]).all()


def test_unsupported_arguments_write_nothing_and_the_predicate_agrees(npm):
    from np_modeling_amd import _C, device as D
    a = _a(8, 32, seed=1)
    spare = D.zeros([64])

    def refused(change, m=8):
        call = Call('NT', _a(m, 32, seed=1), 48, 32, SC.EPI_BIAS)
        change(call.g)
        assert call.run(expect=UNSUPPORTED) is None
        assert b'npm_sgemm_skinny' in _C.lib().npm_last_error()

    refused(lambda g: setattr(g, 'trans_a', 1))                           # TN
    refused(lambda g: setattr(g, 'batch0', 2))
    refused(lambda g: setattr(g, 'batch1', 3))
    refused(lambda g: None, m=65)
    refused(lambda g: setattr(g, 'bsum', spare.ptr))
    refused(lambda g: setattr(g, 'colsum', spare.ptr))
    refused(lambda g: setattr(g, 'asum', spare.ptr))
    refused(lambda g: setattr(g, 'rowdot', spare.ptr))
    refused(lambda g: setattr(g, 'split_k', 2))
    refused(lambda g: setattr(g, 'a', g.a + 4))                           # misaligned pointers
    refused(lambda g: setattr(g, 'c', g.c + 8))
    refused(lambda g: setattr(g, 'bias', g.bias + 4))
    refused(lambda g: setattr(g, 'lda', 34))
    refused(lambda g: setattr(g, 'ldc', 44))
    refused(lambda g: setattr(g, 'n', 40))
    refused(lambda g: setattr(g, 'k', 24))
    refused(lambda g: setattr(g, 'epilogue', 8))                          # NPM_EPI_RELU_MASK
    refused(lambda g: setattr(g, 'epilogue', 32))
    refused(lambda g: setattr(g, 'epilogue', SC.EPI_RELU | SC.EPI_RELU_SAVE))
    ok = Call('NT', a, 48, 32, SC.EPI_BIAS)
    c, _ = ok.run()
    ok.check(c, None, 'the unchanged call')
    assert _C.lib().npm_sgemm_skinny(None) == 10002


# ---- layers ---------------------------------------------------------------------------------------------------------------------
def _layer_close(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    frac = float((np.abs(got - want) / (tol * (np.abs(want) + max(np.abs(want).max(), 1.0)))).max())
    print(f'{what}: {frac:.3f} of {tol:.1e} (|ref| + max |ref|)')
    assert frac <= 1.0, f'{what}: {frac:.3g} of the bound {tol:.3g}'


def _both_routes(npm, run, only=True):
    """``run()`` with SKINNY_GEMM on and off in this process -> (on, off); asserts which GEMM kernels ran (``only``: every product
    of ``run`` is a decode-path product, so with the switch on npm_sgemm does not run at all)."""
    from np_modeling_amd import _C
    D = npm.device
    out = {}
    saved = D.SKINNY_GEMM
    try:
        for on in (True, False):
            D.SKINNY_GEMM = on
            before = _C.last_skinny_kernel()
            with D.KernelTimer() as timer:
                out[on] = run()
            names = set(timer.summary())
            skinny = {n for n in names if n.startswith('sgemm_skinny_')}
            if on:
                assert skinny and not (only and names & {'sgemm_NT', 'sgemm_NN'}), names
                assert _C.last_skinny_kernel().startswith('sgemm_skinny_kernel ')
            else:
                assert not skinny and 'sgemm_NT' in names, names
                assert _C.last_skinny_kernel() == before
    finally:
        D.SKINNY_GEMM = saved
    return out[True], out[False]


@pytest.mark.parametrize('kind', ['contiguous', 'ragged', 'paged'])
@pytest.mark.parametrize('heads,kv_heads,f', [(8, 8, 1024), (8, 2, 1024), (4, 2, 64)])
def test_attention_with_a_cache_on_both_routes(npm, heads, kv_heads, f, kind):
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads + f, batch=3)
    if kind == 'contiguous':
        schedule = [np.array(n) for n in ([5, 5, 5], [1, 1, 1], [1, 1, 1], [3, 3, 3], [1, 1, 1])]
    else:
        schedule = [np.array(n) for n in ([5, 2, 9], [1, 1, 1], [1, 0, 1], [3, 1, 2], [1, 1, 1])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(f)
    x_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    want = VR.layer_alone(p, x_rows, schedule)
    paged = dict(page_size=16) if kind == 'paged' else {}

    def run():
        cache = att.make_cache(3, int(total.max()) + 2, **paged)
        outs = []
        for x, n in VR.padded_calls(x_rows, schedule):
            outs.append(np.asarray(att(x, cache=cache, new_lengths=None if kind == 'contiguous' else n)))
        return VR.collect(outs, schedule, 3)

    on, off = _both_routes(npm, run)
    for b in range(3):
        _layer_close(on[b], want[b], SC.LAYER_TOL, f'{kind} H{heads}/{kv_heads} F{f} sequence {b} skinny')
        _layer_close(off[b], want[b], SC.LAYER_TOL, f'{kind} H{heads}/{kv_heads} F{f} sequence {b} npm_sgemm')
        _layer_close(on[b], off[b], 2 * SC.LAYER_TOL, f'{kind} H{heads}/{kv_heads} F{f} sequence {b} skinny vs npm_sgemm')


@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('kv_heads', [None, 2])
def test_decoder_decode_on_both_routes(npm, norm_first, kv_heads):
    from np_modeling_amd import _C
    D = npm.device
    f, s = 256, 21
    dec, p = DC.make_decoder(npm, f, 4, kv_heads, 384, norm_first, True, seed=11, batch=3, seq_kv=23)
    rng = np.random.default_rng(12)
    q, kv = rng.standard_normal([3, s, f]).astype(np.float32), rng.standard_normal([3, 23, f]).astype(np.float32)
    want, _ = DR.decoder_fwd(p, q.astype(np.float64), kv.astype(np.float64), norm_first, mask=DR.causal_mask(s))
    for sizes in DC.chunkings(s):
        on, off = _both_routes(npm, lambda: DC.run_decoder_chunks(dec, q, kv, sizes, capacity=s + 3), only=False)
        _layer_close(on, want, SC.LAYER_TOL, f'decode chunks {sizes[:4]} skinny vs float64')
        _layer_close(off, want, SC.LAYER_TOL, f'decode chunks {sizes[:4]} npm_sgemm vs float64')
        _layer_close(on, off, 2 * SC.LAYER_TOL, f'decode chunks {sizes[:4]} skinny vs npm_sgemm')
    # M = 3 x 21 = 63 rows ran skinny in the first chunking; the memory prefill never does
    before = _C.last_skinny_kernel()
    with D.KernelTimer() as timer:
        state = dec.start_decoding(kv, s + 3)
    assert not any(n.startswith('sgemm_skinny_') for n in timer.summary()) and _C.last_skinny_kernel() == before
    npm.set_math('bf16x3')                                                # another math mode: nothing skinny runs
    with D.KernelTimer() as timer:
        dec.decode(q[:, :1], state)
    names = set(timer.summary())
    assert not any(n.startswith('sgemm_skinny_') for n in names) and 'sgemm_NT' in names and _C.last_skinny_kernel() == before
    assert _C.last_math() == 'bf16x3'
    npm.set_math('f32')
    with D.KernelTimer() as timer:
        dec.decode(q[:, 1:2], state)
    assert {'sgemm_skinny_NT', 'sgemm_skinny_NN'} <= set(timer.summary())
    assert _C.last_skinny_kernel().startswith('sgemm_skinny_kernel NN M=3 N=256 K=384 rb=1 ')
