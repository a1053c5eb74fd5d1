"""GPU: the fused attention kernels (csrc/npm_attn.hip) where O(1) data does not reach -- the lazy reference point of the
online softmax (A), large and shifted scores (B), long sequences and the 64-tile edge of tile skipping (C), key padding
with key blocks that no query sees (D), and the forward's scheduling knobs (E) -- through the C ABI against the float64
reference of tests/attn_range_data.py (the oracle's formulas, one (b, h) plane at a time).

The bound.  The kernels form every probability as p = 2^e with e = fma(s, c, -m) in the forward (c = scale log2(e) in
float32, m the row's reference point) and e = fma(s, c, -lse log2(e)) in the backward, lse having gone to natural units
and back (npm_attn.hip: the lse store of both forward kernels, mha_rowterms_kernel / mha_lse2_kernel).  Each of those
steps rounds a quantity of magnitude up to X = max |s c| + max |lse log2(e)| (log2 units; |s| taken as scale sum_d |q_d k_d|,
which also bounds the rounding of a score summed from cancelling terms), so e carries an absolute error of a few ulps of X,
a ~ eps X with eps = 2^-24, and p a relative error ln(2) a eps X.  ctx = sum p v / sum p, lse, dq, dk and dv are sums of
p-weighted terms: their errors, in this suite's metric |got - ref| <= tol (|ref| + max |ref|), grow in proportion to that
relative error.  The other rounding (the fp32 products and sums of O(1) operands) does not depend on X.  The existing
bounds tol0 = 2e-6 (ctx) and 3e-6 (lse, gradients) hold on O(1) data, whose X stays below X0 = 32; they therefore cover
the X-dependent part up to X0, and above it the bound grows with it:

    tol(X) = tol0 * max(1, X / X0)

It is tol0 exactly for O(1) scores, and tests/test_attn_range_host.py checks that a float32 evaluation of the same
formulas stays inside it for shifted and saturated data.  Groups A, C, D and E have X <= ~150 (A) or O(1) data.
"""

import ctypes as C
import json
import os

import numpy as np
import pytest

import attn_range_data as R

pytestmark = pytest.mark.gpu

GUARD = 64
BWD = {'bwd8': 3, 'default': 2, 'bwd16': 1, 'bwd4': 0}
FWD = {'fwd8': 2, 'fwd4': 0}
WORST = {}                                               # group -> worst observed fraction of the bound


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    yield np_modeling_amd
    path = os.environ.get('NPM_ATTN_RANGE_REPORT')       # optional: where to write the worst fractions per group
    if path:
        with open(path, 'w') as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _defaults_afterwards(npm):
    """Every knob a test sets (stagger 11, backward 14, forward 17) is back at its default afterwards, however it ended."""
    yield
    from np_modeling_amd import _C
    for knob, value in ((11, 1), (14, 2), (17, 2)):
        _C.check(_C.lib().npm_set_tuning(knob, value), 'npm_set_tuning')


def _tune(knob, value):
    from np_modeling_amd import _C
    _C.check(_C.lib().npm_set_tuning(knob, value), 'npm_set_tuning')


def _guarded(arr, n):
    """The first n elements of a device buffer; the GUARD behind them must still hold the sentinel."""
    np.testing.assert_array_equal(arr.flat_view(n, [arr.size - n]).numpy(), 777.0)
    return arr.flat_view(0, [n]).numpy()


def _run(q, k, v, scale, dctx=None, mask=None, save=False, skip=True, grouped=True, fwd=2, bwd=2, want_scores=False):
    """q / dctx [B,Sq,Hq,D], k / v [B,Skv,Hkv,D] host arrays -> dict of host results, through the grouped entry points
    (``grouped``) or the ungrouped ones (Hkv == Hq).  ``skip``: hand the mask's tile summary to the kernels.  ``fwd`` /
    ``bwd``: NPM_TUNE_ATTN_FWD8 / _BWD16.  The backward runs from the forward's own ctx and lse."""
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    _tune(17, fwd)
    _tune(14, bwd)
    b, sq, h, d = q.shape
    skv, hkv = k.shape[1], k.shape[2]
    assert grouped or hkv == h
    qd, kd, vd = D.from_host(q), D.from_host(k), D.from_host(v)
    ctx = D.full([b * sq * h * d + GUARD], 777.0)
    lse = D.full([b * h * sq + GUARD], 777.0)
    c = _C.npm_mha_core()
    c.batch, c.heads, c.seq_q, c.seq_kv, c.head_dim, c.scale = b, h, sq, skv, d, scale
    c.q, c.k, c.v = qd.ptr, kd.ptr, vd.ptr
    c.q_pitch, c.k_pitch, c.v_pitch = h * d, hkv * d, hkv * d
    c.ctx, c.ctx_pitch, c.lse = ctx.ptr, h * d, lse.ptr
    mask_dev = None
    if mask is not None:
        mask_dev = D.AttnMask(mask, b, h, sq, skv)
        c.mask = mask_dev.buf.ptr
        c.mask_stride_b, c.mask_stride_h, c.mask_stride_q = mask_dev.strides
        if skip:
            assert mask_dev.summary is not None
            c.tile_summary = mask_dev.summary.ptr
            c.summary_stride_b, c.summary_stride_h = mask_dev.summary_strides
            c.summary_all_offset = mask_dev.summary_all_offset
    scores = D.full([b * h * sq * skv + GUARD], 777.0) if save else None
    if save:
        c.scores = scores.ptr

    def call(fn):
        return getattr(lib, fn + '_grouped')(C.byref(c), hkv) if grouped else getattr(lib, fn)(C.byref(c))

    _C.check(call('npm_mha_core_fwd'), 'npm_mha_core_fwd')
    out = {'kernel_fwd': _C.last_attn_kernel()}
    out['ctx'] = _guarded(ctx, b * sq * h * d).reshape(b, sq, h, d)
    out['lse'] = _guarded(lse, b * h * sq).reshape(b, h, sq)
    if save:
        raw = _guarded(scores, b * h * sq * skv) if want_scores else None
        if not want_scores:
            np.testing.assert_array_equal(scores.flat_view(b * h * sq * skv, [GUARD]).numpy(), 777.0)
        out['scores'] = raw
    if dctx is None:
        return out
    views = [D.full([b * s * n * d + GUARD], 777.0) for s, n in ((sq, h), (skv, hkv), (skv, hkv))]
    dctx_d = D.from_host(dctx)
    c.dctx, c.dctx_pitch = dctx_d.ptr, h * d
    c.dq, c.dk, c.dv = (x.ptr for x in views)
    c.dq_pitch, c.dk_pitch, c.dv_pitch = h * d, hkv * d, hkv * d
    _C.check(call('npm_mha_core_bwd'), 'npm_mha_core_bwd')
    out['kernel_bwd'] = _C.last_attn_kernel()
    for name, x, s, n in zip(('dq', 'dk', 'dv'), views, (sq, skv, skv), (h, hkv, hkv)):
        out[name] = _guarded(x, b * s * n * d).reshape(b, s, n, d)
    return out


def _close(group, got, want, tol, what):
    """tests/test_gpu_gqa.py's metric -- |got - ref| <= tol (|ref| + max(max |ref|, 1)) -- and the fraction of it used."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), f'{what}: not finite'
    frac = float((np.abs(got - want) / (tol * (np.abs(want) + max(np.abs(want).max(), 1.0)))).max())
    WORST[group] = max(WORST.get(group, 0.0), frac)
    assert frac <= 1.0, f'{what}: {frac:.3g} of the bound {tol:.3g}'


def _lse_close(group, got, want, tol, what):
    frac = float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / tol)
    WORST[group] = max(WORST.get(group, 0.0), frac)
    assert frac <= 1.0, f'{what} lse: {frac:.3g} of the bound {tol:.3g}'


def _check(group, got, want, x, what, grads=True, kgrow=1.0):
    """ctx, lse (and the gradients) within tol(X); dq within tol(X) kgrow (see test_shift_invariance)."""
    _close(group, got['ctx'], want['ctx'], R.exponent_tol(2e-6, x), f'{what} ctx')
    _lse_close(group, got['lse'], want['lse'], R.exponent_tol(3e-6, x), what)
    if grads:
        for name in ('dq', 'dk', 'dv'):
            _close(group, got[name], want[name], R.exponent_tol(3e-6, x) * (kgrow if name == 'dq' else 1.0), f'{what} {name}')


# ---- A: the lazy reference point ------------------------------------------------------------------------------------
LAZY_SHAPE = (2, 4, 100, 300)          # B, Hq, Sq, Skv (tests/test_attn_range_host.py checks the constructions at it)
MASK_MODES = ('none', 'summary', 'mask only')


@pytest.mark.parametrize('fwd', list(FWD))
@pytest.mark.parametrize('d', [16, 32, 64, 128])
def test_lazy_reference_point(npm, d, fwd):
    """Rows that climb past the threshold on every tile, stay just under it, share a wave with climbers (alpha in
    [2^-10, 1) without triggering), peak in the ragged last or only the first tile, or hide their largest scores and their
    first tiles behind the mask: ctx and lse against the reference for Hkv = Hq and Hkv < Hq, without a mask, with a mask
    and its tile summary and with a mask alone, scores saved and recomputed; then dq, dk, dv from the kernel's own ctx and
    lse under each backward (head size 128 with saved scores; 16 and 64 in both score modes)."""
    b, h, sq, skv = LAZY_SHAPE
    bwd_saves = {128: (True,), 16: (False, True), 64: (False, True)}.get(d, ())
    for hkv in (h, 2):
        for mode in MASK_MODES:
            q, k, v, dctx, scale, mask = R.lazy_problem(b, h, hkv, sq, skv, d, 11 + d + hkv, mode != 'none')
            want = R.reference(q, k, v, dctx, scale, mask)
            x = R.exponent_magnitude(q, k, scale, want['lse'])
            for save in (False, True):
                what = f'hkv={hkv} {mode} save={save}'
                got = _run(q, k, v, scale, mask=mask, save=save, skip=mode == 'summary', grouped=hkv != h, fwd=FWD[fwd])
                assert got['kernel_fwd'].startswith('mha_fwd8_kernel' if fwd == 'fwd8' else 'mha_fwd_kernel')
                _check('A', got, want, x, what, grads=False)
                if save not in bwd_saves:
                    continue
                for name, knob in BWD.items():
                    got = _run(q, k, v, scale, dctx=dctx, mask=mask, save=save, skip=mode == 'summary', grouped=hkv != h,
                               fwd=FWD[fwd], bwd=knob)
                    _check('A', got, want, x, f'{what} {name}')


# ---- B: magnitude and shift invariance ------------------------------------------------------------------------------
@pytest.mark.parametrize('fwd', list(FWD))
@pytest.mark.parametrize('d', [64, 128])
def test_shift_invariance(npm, d, fwd):
    """k_j + u for every key of a (b, K / V head): row i's scores move by scale q_i . u (up to +-200 natural units), lse by
    exactly that, and nothing else changes -- against the unshifted run (each within its bound: the sum of the two) and
    against the reference of the shifted problem.

    dq_i = sum_j dS_ij (k_j + u): the per-probability relative errors (module docstring) no longer cancel in
    sum_j dS_ij u, so the error of dq grows with the size of the keys it is summed from, max |k + u| / max |k|, on top of
    tol(X) -- the factor ``kgrow`` of _check.  ctx, lse, dk and dv have no such term."""
    b, h, hkv, sq, skv = 2, 4, 2, 96, 200
    q, k, v, dctx, scale, ku, shift = R.shift_problem(b, h, hkv, sq, skv, d, 21 + d)
    base_want, want = R.reference(q, k, v, dctx, scale), R.reference(q, ku, v, dctx, scale)
    x0, x = R.exponent_magnitude(q, k, scale, base_want['lse']), R.exponent_magnitude(q, ku, scale, want['lse'])
    assert x > 10 * R.X0
    kgrow = float(np.abs(ku).max() / np.abs(k).max())
    for save in (False, True):
        for name in ('bwd8', 'default', 'bwd4'):
            base = _run(q, k, v, scale, dctx=dctx, save=save, fwd=FWD[fwd], bwd=BWD[name])
            got = _run(q, ku, v, scale, dctx=dctx, save=save, fwd=FWD[fwd], bwd=BWD[name])
            what = f'save={save} {name}'
            _check('B', got, want, x, what, kgrow=kgrow)
            pair = R.exponent_tol(2e-6, x) + R.exponent_tol(2e-6, x0)
            _close('B', got['ctx'], base['ctx'], pair, f'{what} ctx vs unshifted')
            for g in ('dq', 'dk', 'dv'):
                grow = kgrow if g == 'dq' else 1.0
                _close('B', got[g], base[g], R.exponent_tol(3e-6, x) * grow + R.exponent_tol(3e-6, x0), f'{what} {g} vs unshifted')
            _lse_close('B', got['lse'] - base['lse'], shift, R.exponent_tol(3e-6, x) + R.exponent_tol(3e-6, x0), f'{what} shift')


@pytest.mark.parametrize('fwd', list(FWD))
@pytest.mark.parametrize('d', [64, 128])
def test_saturated_softmax(npm, d, fwd):
    """Scaled scores of standard deviation 30: most rows nearly one-hot."""
    b, h, hkv, sq, skv = 2, 4, 2, 96, 200
    q, k, v, dctx, scale = R.saturated_problem(b, h, hkv, sq, skv, d, 31 + d)
    want = R.reference(q, k, v, dctx, scale)
    x = R.exponent_magnitude(q, k, scale, want['lse'])
    for save in (False, True):
        for name in ('bwd8', 'default', 'bwd4'):
            got = _run(q, k, v, scale, dctx=dctx, save=save, fwd=FWD[fwd], bwd=BWD[name])
            _check('B', got, want, x, f'saturated save={save} {name}')


# ---- C: long sequences and the 64-tile edge -------------------------------------------------------------------------
def _causal(sq, skv):
    return np.tril(np.ones([sq, skv], dtype=bool))[None, None]


LONG = {  # name: (B, Hq, Hkv, Sq, Skv, mask)
    'gap 2048': (1, 2, 1, 2048, 2048, lambda: R.gap_mask(2048)),       # rows that see only tile 63, after a long gap
    'causal 2048': (1, 2, 2, 2048, 2048, lambda: _causal(2048, 2048)),  # 16 query tiles: pairing
    'gap 2049': (1, 2, 2, 2049, 2049, lambda: R.gap_mask(2049)),        # beyond 2048: no tile skipping
    'causal 2080': (1, 2, 1, 2080, 2080, lambda: _causal(2080, 2080)),
    'plain 4100': (1, 1, 1, 4100, 4100, lambda: None),
    'causal 4100': (1, 1, 1, 4100, 4100, lambda: _causal(4100, 4100)),
    'wide 16405': (1, 2, 1, 40, 16384 + 21, lambda: None),               # 513 key tiles, ragged tail; 129 / 65 backward key blocks
}


@pytest.mark.parametrize('d', [64, 128])
@pytest.mark.parametrize('case', list(LONG))
def test_long_sequences(npm, case, d):
    """Every forward kernel; bwd8, the default and bwd4; both score modes.  Masked cases with and without the tile summary:
    at 2048 both against the reference, above 2048 (where the summary is ignored) bit-identical to each other."""
    b, h, hkv, sq, skv, make_mask = LONG[case]
    mask = make_mask()
    assert b * h * sq * skv <= 2 ** 25
    rng = np.random.default_rng(sq + skv + d)
    q = rng.standard_normal([b, sq, h, d]).astype(np.float32)
    k, v = (rng.standard_normal([b, skv, hkv, d]).astype(np.float32) for _ in range(2))
    dctx = rng.standard_normal([b, sq, h, d]).astype(np.float32)
    scale = 1.0 / np.sqrt(d)
    want = R.reference(q, k, v, dctx, scale, mask)
    x = R.exponent_magnitude(q, k, scale, want['lse'])
    for save in (False, True):
        got = _run(q, k, v, scale, mask=mask, save=save, fwd=0)
        _check('C', got, want, x, f'{case} save={save} fwd4', grads=False)
        for name in ('bwd8', 'default', 'bwd4'):
            got = _run(q, k, v, scale, dctx=dctx, mask=mask, save=save, bwd=BWD[name])
            _check('C', got, want, x, f'{case} save={save} {name}')
            if mask is None:
                continue
            plain = _run(q, k, v, scale, dctx=dctx, mask=mask, save=save, skip=False, bwd=BWD[name])
            if sq > 2048:
                for g in ('ctx', 'lse', 'dq', 'dk', 'dv'):
                    np.testing.assert_array_equal(plain[g], got[g], err_msg=f'{case} {g} summary ignored')
            else:
                _check('C', plain, want, x, f'{case} save={save} {name} without summary')


# ---- D: key padding -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [16, 64, 128])
def test_key_padding(npm, d):
    """[B, 1, 1, Skv] with valid lengths (700, 384, 300, 129): whole hidden 128- and 256-key blocks, a 256-key block whose
    second half is hidden, a block with one visible key.  dk = dv = exactly 0 on hidden keys (written, not left alone),
    everything else against the reference; every backward, with and without the summary, both score modes, grouped and
    ungrouped calls."""
    b, h, sq, skv = 4, 4, 160, 700
    mask = R.key_padding_mask(R.PAD_LENGTHS, skv)
    hidden = ~mask[:, 0, 0]                                                       # [B, Skv]
    for hkv in (h, 2):
        rng = np.random.default_rng(d + hkv)
        q = rng.standard_normal([b, sq, h, d]).astype(np.float32)
        k, v = (rng.standard_normal([b, skv, hkv, d]).astype(np.float32) for _ in range(2))
        dctx = rng.standard_normal([b, sq, h, d]).astype(np.float32)
        scale = 1.0 / np.sqrt(d)
        want = R.reference(q, k, v, dctx, scale, mask)
        x = R.exponent_magnitude(q, k, scale, want['lse'])
        for skip in (True, False):
            for save in (False, True):
                for name, knob in BWD.items():
                    got = _run(q, k, v, scale, dctx=dctx, mask=mask, save=save, skip=skip, grouped=hkv != h, bwd=knob)
                    what = f'hkv={hkv} skip={skip} save={save} {name}'
                    for g in ('dk', 'dv'):
                        assert (got[g][hidden] == 0).all(), f'{what} {g} on hidden keys'
                    _check('D', got, want, x, what)


@pytest.mark.parametrize('kv_heads', [None, 2])
@pytest.mark.parametrize('d', [64, 128])
def test_layer_key_padding(npm, d, kv_heads):
    """MultiHeadAttention(num_heads, num_kv_heads)(x, mask=key padding): forward, input gradient and SGD update against
    the float64 restatement (tests/gqa_reference.py, which is the reference MHA for num_kv_heads = None)."""
    from test_gpu_gqa import _check_layer
    heads, s = 4, 700
    _check_layer(npm, heads, kv_heads, heads * d, 4, s, None, 40 + d, mask=R.key_padding_mask(R.PAD_LENGTHS, s))


# ---- E: scheduling knobs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fwd', list(FWD))
@pytest.mark.parametrize('sq', [384, 512])
def test_schedule_knobs_change_no_bit(npm, sq, fwd):
    """NPM_TUNE_ATTN_STAGGER (11) = 0, 1, 3 and 257 (bit 8: no query-tile pairing, stagger 1) under a causal mask with its
    tile summary, at an odd (3) and an even (4) number of 128-query tiles: ctx, lse and the saved scores bit-equal to the
    default's.  The fixture puts the default (1) back."""
    b, h, d = 2, 2, 64
    rng = np.random.default_rng(sq)
    q = rng.standard_normal([b, sq, h, d]).astype(np.float32)
    k, v = (rng.standard_normal([b, sq, h, d]).astype(np.float32) for _ in range(2))
    mask = R.gap_mask(sq)
    ref = _run(q, k, v, 0.125, mask=mask, save=True, grouped=False, fwd=FWD[fwd], want_scores=True)
    want = R.reference(q, k, v, None, 0.125, mask, grads=False)
    _check('E', ref, want, R.exponent_magnitude(q, k, 0.125, want['lse']), f'sq={sq}', grads=False)
    for value in (0, 1, 3, 257):
        _tune(11, value)
        got = _run(q, k, v, 0.125, mask=mask, save=True, grouped=False, fwd=FWD[fwd], want_scores=True)
        for name in ('ctx', 'lse', 'scores'):
            np.testing.assert_array_equal(got[name], ref[name], err_msg=f'stagger {value} {name}')
