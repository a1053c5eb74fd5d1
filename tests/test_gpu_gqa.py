"""GPU: grouped-query attention -- the fused kernels' grouped entry points (npm_mha_core_fwd_grouped / _bwd_grouped,
csrc/npm_attn.hip) through the C ABI, MultiHeadAttention(num_heads, num_kv_heads=...) on the fused core and on the GEMM
composition, and the encoder / decoder with num_kv_heads -- against the float64 restatement of the reference's gqa_fwd
(tests/gqa_reference.py; layers/attentions_test.py:267-358)."""

import copy
import ctypes as C

import numpy as np
import pytest

import gqa_reference as G
from conftest import assert_close as _assert_close
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

NPM_E_BAD_ARGUMENT = 10002
_MHA = ['wq', 'wk', 'wv', 'wo', 'bq', 'bk', 'bv', 'bo']


def assert_close(got, ref, tol=1e-5, what=''):
    """conftest's metric with a floor on the scale (as tests/test_gpu_attn.py: operands here are O(1))."""
    ref = np.asarray(ref, dtype=np.float64)
    if ref.size and np.abs(ref).max() < 1.0:
        np.testing.assert_allclose(np.asarray(got, dtype=np.float64), ref, rtol=tol, atol=tol, err_msg=what)
    else:
        _assert_close(got, ref, tol=tol, what=what)


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.fixture
def tuning(npm):
    """Selects the attention backward (NPM_TUNE_ATTN_BWD16 = 14) and forward (NPM_TUNE_ATTN_FWD8 = 17) kernels the way
    tests/test_gpu_attn.py's fixtures do; back to the defaults afterwards."""
    from np_modeling_amd import _C

    def select(bwd, fwd):
        _C.check(_C.lib().npm_set_tuning(14, bwd), 'npm_set_tuning')
        _C.check(_C.lib().npm_set_tuning(17, fwd), 'npm_set_tuning')
    yield select
    select(2, 2)


# ---- the core through the C ABI ----------------------------------------------------------------------------------
def _run(q, k, v, scale, dctx=None, mask=None, save=False, packed=False, neg_delta=None, kv_heads='grouped', lse_ctx=None):
    """q [B,Sq,Hq,D], k / v [B,Skv,Hkv,D] host arrays -> dict of host results.  ``kv_heads``: 'grouped' calls the grouped
    entry points with Hkv, None the ungrouped ones (Hkv == Hq only), an int is passed as is.  ``packed``: q, k, v (and dq, dk,
    dv) in one [B, S, Hq + 2 Hkv, D] buffer.  Every output has a guard region behind it that must stay untouched."""
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    b, sq, h, d = q.shape
    skv, hkv = k.shape[1], k.shape[2]
    guard = 64
    width = (h + 2 * hkv) * d
    if packed:
        assert sq == skv
        dev = D.from_host(np.concatenate([q, k, v], axis=2))
        qd, kd, vd = dev, dev.flat_view(h * d, [dev.size - h * d]), dev.flat_view((h + hkv) * d, [dev.size - (h + hkv) * d])
        pitches = (width, width, width)
    else:
        qd, kd, vd = D.from_host(q), D.from_host(k), D.from_host(v)
        pitches = (h * d, hkv * d, hkv * d)
    ctx = D.full([b * sq * h * d + guard], 777.0)
    lse = D.full([b * h * sq + guard], 777.0)
    c = _C.npm_mha_core()
    c.batch, c.heads, c.seq_q, c.seq_kv, c.head_dim, c.scale = b, h, sq, skv, d, scale
    c.q, c.k, c.v = qd.ptr, kd.ptr, vd.ptr
    c.q_pitch, c.k_pitch, c.v_pitch = pitches
    c.ctx, c.ctx_pitch, c.lse = ctx.ptr, h * d, lse.ptr
    mask_dev = None
    if mask is not None:
        mask_dev = D.AttnMask(mask, b, h, sq, skv)
        c.mask = mask_dev.buf.ptr
        c.mask_stride_b, c.mask_stride_h, c.mask_stride_q = mask_dev.strides
        if mask_dev.summary is not None:
            c.tile_summary = mask_dev.summary.ptr
            c.summary_stride_b, c.summary_stride_h = mask_dev.summary_strides
            c.summary_all_offset = mask_dev.summary_all_offset
    scores = D.full([b * h * sq * skv + guard], 777.0) if save else None
    if save:
        c.scores = scores.ptr
    nkv = hkv if kv_heads == 'grouped' else kv_heads

    def call(fn):
        if nkv is None:
            return getattr(lib, fn)(C.byref(c))
        return getattr(lib, fn + '_grouped')(C.byref(c), nkv)

    rc = call('npm_mha_core_fwd')
    out = {'rc_fwd': rc}
    if rc:
        return out
    out['kernel_fwd'] = _C.last_attn_kernel()
    for key, arr, n in (('ctx', ctx, b * sq * h * d), ('lse', lse, b * h * sq)):
        raw = arr.numpy()
        np.testing.assert_array_equal(raw[n:], 777.0)
        out[key] = raw[:n]
    out['ctx'] = out['ctx'].reshape(b, sq, h, d)
    out['lse'] = out['lse'].reshape(b, h, sq)
    if dctx is None:
        return out
    if lse_ctx is not None:                                  # the restatement's forward results: isolates the backward
        ctx.flat_view(0, [b, sq, h, d]).set(lse_ctx[1])
        lse.flat_view(0, [b, h, sq]).set(lse_ctx[0])
    if packed:
        gbuf = D.full([b * sq * width + guard], 777.0)
        views = [gbuf, gbuf.flat_view(h * d, [gbuf.size - h * d]), gbuf.flat_view((h + hkv) * d, [gbuf.size - (h + hkv) * d])]
        gp = (width,) * 3
    else:
        views = [D.full([b * s * n * d + guard], 777.0) for s, n in ((sq, h), (skv, hkv), (skv, hkv))]
        gp = (h * d, hkv * d, hkv * d)
    dctx_d = D.from_host(dctx)
    c.dctx, c.dctx_pitch = dctx_d.ptr, h * d
    c.dq, c.dk, c.dv = (x.ptr for x in views)
    c.dq_pitch, c.dk_pitch, c.dv_pitch = gp
    if neg_delta is not None:                                # [Hq, B, Sq]
        nd = D.from_host(neg_delta)
        c.neg_delta, c.neg_delta_stride_b, c.neg_delta_stride_h = nd.ptr, neg_delta.shape[2], neg_delta.shape[1] * neg_delta.shape[2]
    rc = call('npm_mha_core_bwd')
    out['rc_bwd'] = rc
    if rc:
        return out
    out['kernel_bwd'] = _C.last_attn_kernel()
    if packed:
        raw = gbuf.numpy()
        np.testing.assert_array_equal(raw[b * sq * width:], 777.0)
        g = raw[:b * sq * width].reshape(b, sq, h + 2 * hkv, d)
        out.update(dq=g[:, :, :h], dk=g[:, :, h:h + hkv], dv=g[:, :, h + hkv:])
    else:
        for name, x, s, n in zip(('dq', 'dk', 'dv'), views, (sq, skv, skv), (h, hkv, hkv)):
            raw = x.numpy()
            np.testing.assert_array_equal(raw[b * s * n * d:], 777.0)
            out[name] = raw[:b * s * n * d].reshape(b, s, n, d)
    return out


def _data(seed, b, h, hkv, sq, skv, d):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal([b, sq, h, d]).astype(np.float32)
    k = rng.standard_normal([b, skv, hkv, d]).astype(np.float32)
    v = rng.standard_normal([b, skv, hkv, d]).astype(np.float32)
    dctx = rng.standard_normal([b, sq, h, d]).astype(np.float32)
    return rng, q, k, v, dctx


def _want(q, k, v, dctx, scale, mask=None):
    """The restatement at the core level: query head h with K / V head h % Hkv (tests/test_gqa_host.py pins that this is
    gqa_fwd's mapping); dk / dv are the group sums."""
    h, hkv = q.shape[2], k.shape[2]
    q64, kf, vf, d64 = q.astype(np.float64), G.expand_kv(k.astype(np.float64), h), G.expand_kv(v.astype(np.float64), h), dctx.astype(np.float64)
    full = None if mask is None else np.broadcast_to(mask, (q.shape[0], h, q.shape[1], k.shape[1]))
    ctx, lse, probs = O.attention_core_fwd(q64, kf, vf, scale, full) if full is not None else O.attention_core_fwd(q64, kf, vf, scale)
    dq, dkf, dvf = O.attention_core_bwd(q64, kf, vf, probs, d64, scale)
    return dict(ctx=ctx, lse=lse, dq=dq, dk=G.group_sum(dkf, hkv), dv=G.group_sum(dvf, hkv))


CORE_SHAPES = [  # b, hq, hkv, sq, skv, d
    (2, 2, 1, 33, 47, 16), (1, 8, 2, 130, 257, 16), (2, 4, 2, 47, 33, 32), (1, 8, 1, 257, 130, 64),
    (2, 8, 4, 64, 64, 128), (1, 8, 1, 130, 257, 128), (1, 4, 1, 128, 128, 32),
]
BWD_KERNELS = {3: 'mha_bwd8_kernel', 1: None, 0: 'mha_bwd_kernel'}


@pytest.mark.parametrize('bwd', [3, 2, 1, 0], ids=['bwd8', 'default', 'bwd16', 'bwd4'])
@pytest.mark.parametrize('fwd', [2, 0], ids=['fwd8', 'fwd4'])
@pytest.mark.parametrize('b,h,hkv,sq,skv,d', CORE_SHAPES)
def test_core_vs_restatement(npm, tuning, b, h, hkv, sq, skv, d, bwd, fwd):
    """Every head size, G in {2, 4, 8} (Hkv = 1 included), Sq != Skv and ragged lengths, every forward and backward kernel,
    scores saved and recomputed."""
    tuning(bwd, fwd)
    _, q, k, v, dctx = _data(b * 1000 + h * 100 + hkv * 10 + sq + skv + d, b, h, hkv, sq, skv, d)
    scale = 1.0 / np.sqrt(d)
    want = _want(q, k, v, dctx, scale)
    for save in (False, True):
        got = _run(q, k, v, scale, dctx=dctx, save=save)
        assert got['rc_fwd'] == 0 and got['rc_bwd'] == 0
        assert got['kernel_fwd'].startswith('mha_fwd8_kernel' if fwd == 2 else 'mha_fwd_kernel')
        assert got['kernel_fwd'].endswith(f' kv_heads={hkv}') and got['kernel_bwd'].endswith(f' kv_heads={hkv}')
        if BWD_KERNELS.get(bwd):
            assert got['kernel_bwd'].startswith(BWD_KERNELS[bwd])
        assert_close(got['ctx'], want['ctx'], tol=2e-6, what=f'ctx save={save}')
        np.testing.assert_allclose(got['lse'], want['lse'], rtol=0, atol=3e-6)
        for name in ('dq', 'dk', 'dv'):
            assert_close(got[name], want[name], tol=3e-6, what=f'{name} save={save}')
    if bwd == 2 and fwd == 2:                                # the backward on its own (the restatement's lse / ctx)
        got = _run(q, k, v, scale, dctx=dctx, lse_ctx=(want['lse'], want['ctx']))
        for name in ('dq', 'dk', 'dv'):
            assert_close(got[name], want[name], tol=3e-6, what=name)


@pytest.mark.parametrize('b,h,hkv,sq,skv,d', [(2, 6, 2, 70, 90, 32), (1, 16, 1, 33, 130, 64), (2, 12, 4, 64, 48, 128)])
def test_core_group_sizes_of_the_generic_reduce(npm, b, h, hkv, sq, skv, d):
    """G = 3 and 16: the reduce kernel's run-time group loop (G = 2, 4, 8 have instances of their own)."""
    _, q, k, v, dctx = _data(h * 31 + sq + d, b, h, hkv, sq, skv, d)
    scale = 1.0 / np.sqrt(d)
    want = _want(q, k, v, dctx, scale)
    got = _run(q, k, v, scale, dctx=dctx, save=d >= 64)
    assert_close(got['ctx'], want['ctx'], tol=2e-6)
    for name in ('dq', 'dk', 'dv'):
        assert_close(got[name], want[name], tol=3e-6, what=name)


@pytest.mark.parametrize('bwd', [2, 0], ids=['default', 'bwd4'])
@pytest.mark.parametrize('b,h,hkv,sq,skv,d', [(2, 4, 2, 40, 70, 16), (1, 8, 2, 130, 130, 128), (2, 4, 1, 64, 33, 32)])
def test_core_masked(npm, tuning, b, h, hkv, sq, skv, d, bwd):
    """Causal, random and per-head masks (one plane per QUERY head), each with its tile summary, scores saved and not."""
    tuning(bwd, 2)
    rng, q, k, v, dctx = _data(sq + skv + d, b, h, hkv, sq, skv, d)
    scale = 1.0 / np.sqrt(d)
    causal = np.tril(np.ones([sq, skv], dtype=bool))[None, None]
    random = rng.random([b, h, sq, skv]) < 0.6
    random[..., 0] = True
    per_head = rng.random([1, h, 1, skv]) < 0.7
    per_head[..., 3] = True
    for kind, mask in (('causal', causal), ('random', random), ('per head', per_head)):
        want = _want(q, k, v, dctx, scale, mask)
        for save in (False, True):
            got = _run(q, k, v, scale, dctx=dctx, mask=mask, save=save)
            assert_close(got['ctx'], want['ctx'], tol=2e-6, what=kind)
            np.testing.assert_allclose(got['lse'], want['lse'], rtol=0, atol=3e-6)
            for name in ('dq', 'dk', 'dv'):
                assert_close(got[name], want[name], tol=3e-6, what=f'{kind} {name} save={save}')


@pytest.mark.parametrize('b,h,hkv,sq,skv,d', [(2, 4, 2, 64, 96, 128), (1, 8, 1, 36, 70, 64), (2, 4, 2, 33, 47, 16)])
def test_core_row_terms_from_the_caller(npm, b, h, hkv, sq, skv, d):
    """``neg_delta`` (per query head, [Hq, B, Sq]) with the grouped backward."""
    _, q, k, v, dctx = _data(b + h + sq + d, b, h, hkv, sq, skv, d)
    scale = 1.0 / np.sqrt(d)
    want = _want(q, k, v, dctx, scale)
    terms = (-scale * np.einsum('bqhd,bqhd->hbq', dctx.astype(np.float64), want['ctx'])).astype(np.float32)
    got = _run(q, k, v, scale, dctx=dctx, save=d >= 64, lse_ctx=(want['lse'], want['ctx']), neg_delta=terms)
    for name in ('dq', 'dk', 'dv'):
        assert_close(got[name], want[name], tol=3e-6, what=name)


@pytest.mark.parametrize('b,h,hkv,s,d', [(2, 4, 2, 96, 16), (1, 8, 2, 160, 128), (2, 8, 1, 64, 64)])
def test_core_packed_operands(npm, b, h, hkv, s, d):
    """q, k, v and their gradients in one [B, S, Hq + 2 Hkv, D] buffer (row pitch (Hq + 2 Hkv) D), scores saved and not."""
    _, q, k, v, dctx = _data(s + d + hkv, b, h, hkv, s, s, d)
    scale = 1.0 / np.sqrt(d)
    want = _want(q, k, v, dctx, scale)
    for save in (False, True):
        got = _run(q, k, v, scale, dctx=dctx, packed=True, save=save)
        assert_close(got['ctx'], want['ctx'], tol=2e-6)
        for name in ('dq', 'dk', 'dv'):
            assert_close(got[name], want[name], tol=3e-6, what=f'{name} save={save}')


@pytest.mark.parametrize('d', [16, 128])
def test_as_many_kv_heads_as_query_heads_is_the_ungrouped_call(npm, d):
    _, q, k, v, dctx = _data(d, 2, 4, 4, 70, 90, d)
    scale = 1.0 / np.sqrt(d)
    for save in (False, True):
        plain = _run(q, k, v, scale, dctx=dctx, save=save, kv_heads=None)
        grouped = _run(q, k, v, scale, dctx=dctx, save=save, kv_heads=4)
        assert grouped['kernel_fwd'] == plain['kernel_fwd'] and 'kv_heads' not in grouped['kernel_fwd']
        assert grouped['kernel_bwd'] == plain['kernel_bwd'] and 'kv_heads' not in grouped['kernel_bwd']
        for name in ('ctx', 'lse', 'dq', 'dk', 'dv'):
            np.testing.assert_array_equal(grouped[name], plain[name], err_msg=name)


def test_grouped_backward_is_bitwise_reproducible(npm):
    _, q, k, v, dctx = _data(5, 2, 8, 2, 128, 200, 64)
    scale = 1.0 / np.sqrt(64)
    first = _run(q, k, v, scale, dctx=dctx)
    second = _run(q, k, v, scale, dctx=dctx)
    for name in ('dq', 'dk', 'dv'):
        np.testing.assert_array_equal(first[name], second[name], err_msg=name)


def test_grouped_backward_without_queries_zeroes_dk_dv(npm):
    """Sq = 0: nothing flows back, dk / dv (Hkv heads wide) are zero and the memory behind them untouched."""
    from np_modeling_amd import _C, device as D
    b, h, hkv, skv, d = 2, 4, 2, 33, 32
    rng = np.random.default_rng(1)
    k = D.from_host(rng.standard_normal([b, skv, hkv, d]).astype(np.float32))
    v = D.from_host(rng.standard_normal([b, skv, hkv, d]).astype(np.float32))
    q, ctx, lse, dctx, dq = (D.full([64], 1.0) for _ in range(5))
    n = b * skv * hkv * d
    dk, dv = D.full([n + 64], 777.0), D.full([n + 64], 777.0)
    c = _C.npm_mha_core()
    c.batch, c.heads, c.seq_q, c.seq_kv, c.head_dim, c.scale = b, h, 0, skv, d, 1.0 / np.sqrt(d)
    c.q, c.k, c.v, c.ctx, c.lse, c.dctx, c.dq, c.dk, c.dv = q.ptr, k.ptr, v.ptr, ctx.ptr, lse.ptr, dctx.ptr, dq.ptr, dk.ptr, dv.ptr
    c.q_pitch = c.ctx_pitch = c.dctx_pitch = c.dq_pitch = h * d
    c.k_pitch = c.v_pitch = c.dk_pitch = c.dv_pitch = hkv * d
    _C.check(_C.lib().npm_mha_core_bwd_grouped(C.byref(c), hkv), 'npm_mha_core_bwd_grouped')
    for x in (dk, dv):
        raw = x.numpy()
        np.testing.assert_array_equal(raw[:n], 0.0)
        np.testing.assert_array_equal(raw[n:], 777.0)


@pytest.mark.parametrize('kv_heads', [0, -1, 3, 5])
def test_bad_kv_heads_is_a_bad_argument(npm, kv_heads):
    _, q, k, v, dctx = _data(2, 1, 4, 2, 16, 16, 16)
    got = _run(q, k, v, 0.25, dctx=dctx, kv_heads=kv_heads)
    assert got['rc_fwd'] == NPM_E_BAD_ARGUMENT
    from np_modeling_amd import _C
    c = _C.npm_mha_core()                                          # the backward rejects it before touching any pointer
    c.batch, c.heads, c.seq_q, c.seq_kv, c.head_dim, c.scale = 1, 4, 16, 16, 16, 0.25
    assert _C.lib().npm_mha_core_bwd_grouped(C.byref(c), kv_heads) == NPM_E_BAD_ARGUMENT


# ---- the layer -------------------------------------------------------------------------------------------------------
def _assign(obj, name, value):
    """Writes a parameter in place: the layer's buffers (the packed in-projections among them) stay where they are."""
    getattr(obj, name).set(value)


def _layer(npm, heads, kv_heads, feat, seed, kv_len=0, rebind=False, **kw):
    """A layer initialised at ``seed`` with its weights scaled by 1 / sqrt(F) (O(1) activations); returns it and the
    parameters it now holds (fp32).  ``rebind``: assign host arrays to the attributes instead (the in-projections are then
    separate buffers, as after a weight binder)."""
    np.random.seed(seed)
    layer = npm.layers.MultiHeadAttention(num_heads=heads, num_kv_heads=kv_heads, **kw)
    probe = np.zeros([1, 4, feat], dtype=np.float32)
    layer(probe, np.zeros([1, 4, feat], dtype=np.float32)) if kv_len else layer(probe)
    p = {}
    for n in _MHA:
        p[n] = (np.asarray(getattr(layer, '_' + n)) / (np.sqrt(feat) if n[0] == 'w' else 1.0)).astype(np.float32)
        if rebind:
            setattr(layer, '_' + n, p[n].copy())
        else:
            _assign(layer, '_' + n, p[n])
    return layer, p


def _check_layer(npm, heads, kv_heads, feat, b, sq, skv, seed, tol=1e-5, mask=None, rebind=False):
    rng = np.random.default_rng(seed)
    cross = skv is not None
    layer, p = _layer(npm, heads, kv_heads, feat, seed, kv_len=skv or 0, rebind=rebind)
    hkv = kv_heads or heads
    assert p['wk'].shape == (hkv, feat // heads, feat) and p['bv'].shape == (hkv, feat // heads)
    query = rng.standard_normal([b, sq, feat]).astype(np.float32)
    kv = rng.standard_normal([b, skv, feat]).astype(np.float32) if cross else None
    dy = rng.standard_normal([b, sq, feat]).astype(np.float32)
    out = layer(query, kv, mask=mask) if cross else layer(query, mask=mask)
    p64 = {n: p[n].astype(np.float64) for n in _MHA}
    mfull = None if mask is None else np.broadcast_to(mask, (b, heads, sq, skv or sq))
    want, cache = G.gqa_fwd(p64, query.astype(np.float64), None if kv is None else kv.astype(np.float64),
                            None if kv is None else kv.astype(np.float64), mfull)
    assert_close(out, want, tol=tol)
    lr = 0.05
    grads = [np.asarray(g) for g in layer(dy, backprop=True, learning_rate=lr)]
    wg, pg = G.gqa_bwd(p64, cache, dy.astype(np.float64))
    if cross:
        assert_close(grads[0], wg[0], tol=tol, what='dquery')
        assert_close(grads[1] + grads[2], wg[1] + wg[2], tol=tol, what='dkey + dvalue')
    else:
        assert_close(sum(grads), sum(wg), tol=tol, what='dx')
    for n in _MHA:
        assert_close(getattr(layer, '_' + n), p64[n] - lr * pg[n], tol=tol, what=n)
    return layer


def test_layer_reference_configuration(npm):
    """attentions_test.py:267-358's own configuration: B 16, S 128, Hq 8, Hkv 4, F 128 -- forward and every gradient."""
    from np_modeling_amd import _C
    layer = _check_layer(npm, 8, 4, 128, 16, 128, None, 0)
    assert layer._core and layer._packed
    assert 'kv_heads=4' in _C.last_attn_kernel()


def test_layer_adam_step(npm):
    """One Adam step (oracle restatement of reference optimizer.py:53-67) on every parameter, from the gradients the layer
    produces (read off a deep copy that takes an SGD step of rate 1 instead: Adam's normalisation would magnify the fp32
    rounding of near-zero gradients against an fp64 reference).  bk is left out: its gradient is zero in exact arithmetic
    (q . bk is the same for every key, and the softmax does not see a constant), so Adam's step on it normalises rounding
    noise that the rate-1 SGD step of the copy cannot resolve."""
    rng = np.random.default_rng(1)
    layer, p = _layer(npm, 8, 2, 128, 1)
    x = rng.standard_normal([4, 64, 128]).astype(np.float32)
    dy = rng.standard_normal([4, 64, 128]).astype(np.float32)
    layer(x)
    twin = copy.deepcopy(layer)
    layer(dy, backprop=True, optimizer_=npm.optimizer.AdamOptimizer(0.05))
    twin(dy, backprop=True, learning_rate=1.0)
    for n in _MHA:
        if n == 'bk':
            continue
        p0 = p[n].astype(np.float64)
        grad = p0 - np.asarray(getattr(twin, '_' + n)).astype(np.float64)
        assert np.abs(grad).max() > 0, n
        assert_close(getattr(layer, '_' + n), O.adam_step(p0, grad, {}, 0.05), tol=2e-6, what=n)


@pytest.mark.parametrize('heads,kv_heads,feat', [(8, 2, 256), (4, 1, 512)])
def test_layer_cross_attention(npm, heads, kv_heads, feat):
    _check_layer(npm, heads, kv_heads, feat, 2, 40, 70, 2)


def test_layer_unpacked_self_attention(npm):
    """Self-attention with the in-projections NOT adjacent in memory: three projection GEMMs, three input-gradient GEMMs."""
    layer = _check_layer(npm, 8, 2, 128, 2, 64, None, 3, rebind=True)
    assert not layer._packed


@pytest.mark.parametrize('mode', ['f32', 'bf16x3'])
@pytest.mark.parametrize('cross', [False, True])
def test_layer_gemm_composition_head_size_8(npm, mode, cross):
    """Dk = 8 (F 64, Hq 8, Hkv 2): no fused kernel takes it, the GEMM composition runs (one batched GEMM per group, dK / dV
    summed in the residual epilogue); under bf16x3 at that mode's bound (include/npm_hip.h NPM_PARITY_SCALED_BF16X3)."""
    npm.set_math(mode)
    try:
        layer = _check_layer(npm, 8, 2, 64, 3, 33, 47 if cross else None, 4)
        assert not layer._core
    finally:
        npm.set_math('f32')


def test_layer_bf16x3_takes_the_composition(npm):
    """Under a split-precision mode the fused head sizes go through the GEMM composition too."""
    npm.set_math('bf16x3')
    try:
        layer = _check_layer(npm, 4, 2, 64, 2, 40, None, 5)
        assert not layer._core
    finally:
        npm.set_math('f32')


def test_layer_masked(npm):
    mask = np.tril(np.ones([48, 48], dtype=bool))[None, None]
    _check_layer(npm, 8, 2, 128, 2, 48, None, 6, mask=mask)


def test_layer_with_num_kv_heads_equal_num_heads_is_mha_bitwise(npm):
    rng = np.random.default_rng(7)
    query = rng.standard_normal([2, 40, 128]).astype(np.float32)
    dy = rng.standard_normal([2, 40, 128]).astype(np.float32)
    results = []
    for kw in ({}, {'num_kv_heads': 8}):
        np.random.seed(11)
        layer = npm.layers.MultiHeadAttention(num_heads=8, **kw)
        out = np.asarray(layer(query))
        grads = [np.asarray(g) for g in layer(dy, backprop=True, learning_rate=0.01)]
        results.append((out, grads, {n: np.asarray(getattr(layer, '_' + n)) for n in _MHA}))
    (o1, g1, p1), (o2, g2, p2) = results
    np.testing.assert_array_equal(o1, o2)
    for a, b_ in zip(g1, g2):
        np.testing.assert_array_equal(a, b_)
    for n in _MHA:
        np.testing.assert_array_equal(p1[n], p2[n], err_msg=n)


def test_layer_rejects_heads_not_divisible_by_kv_heads(npm):
    with pytest.raises(AssertionError):
        npm.layers.MultiHeadAttention(num_heads=8, num_kv_heads=3)(np.zeros([1, 4, 64], dtype=np.float32))


# ---- encoder / decoder -----------------------------------------------------------------------------------------------
_ATT = ['wq', 'wk', 'wv', 'wo', 'bq', 'bk', 'bv', 'bo']


def _pair(npm, cls, heads, kv_heads, seed, init_args, **kw):
    """The grouped composite and an MHA composite holding the same parameters (attention, norms, feed-forward), with the
    grouped one's K / V weights repeated (head h = K / V head h % Hkv).  Weights scaled by 1 / sqrt(fan-in) for O(1)
    activations."""
    np.random.seed(seed)
    gqa = cls(num_heads=heads, num_kv_heads=kv_heads, **kw)
    gqa(*init_args)
    np.random.seed(seed)
    mha = cls(num_heads=heads, **kw)
    mha(*init_args)
    idx = np.arange(heads) % kv_heads
    for attr in ('_self_attention', '_cross_attention'):
        ga, ma = getattr(gqa, attr, None), getattr(mha, attr, None)
        if ga is None:
            continue
        for n in _ATT:
            arr = np.asarray(getattr(ga, '_' + n)).astype(np.float32)
            if n[0] == 'w':
                arr = arr / np.float32(np.sqrt(arr.shape[-1] if n != 'wo' else arr.shape[1] * arr.shape[2]))
            _assign(ga, '_' + n, arr)
            _assign(ma, '_' + n, arr[idx] if n in ('wk', 'wv', 'bk', 'bv') else arr)
    for norm in ('_norm1', '_norm2', '_norm3'):
        if hasattr(gqa, norm):
            for n in ('_gamma', '_beta'):
                _assign(getattr(mha, norm), n, np.asarray(getattr(getattr(gqa, norm), n)))
    for lin in ('_dense1', '_dense2'):
        gl, ml = getattr(gqa, lin), getattr(mha, lin)
        gl, ml = getattr(gl, '_linear', gl), getattr(ml, '_linear', ml)
        for n in ('_w', '_b'):
            arr = np.asarray(getattr(gl, n)).astype(np.float32)
            if n == '_w':
                arr = arr / np.float32(np.sqrt(arr.shape[0]))
            _assign(gl, n, arr)
            _assign(ml, n, arr)
    return gqa, mha


def _compare_attention_params(ga, ma, before, heads, kv_heads, lr):
    """Updated K / V parameters of the grouped layer = before - lr * (group sums of the MHA layer's gradients)."""
    for n in _ATT:
        g_new, m_new = np.asarray(getattr(ga, '_' + n)).astype(np.float64), np.asarray(getattr(ma, '_' + n)).astype(np.float64)
        b0 = before[n].astype(np.float64)
        if n in ('wk', 'wv', 'bk', 'bv'):
            m_grad = (b0[np.arange(heads) % kv_heads] - m_new) / lr
            want = b0 - lr * m_grad.reshape((heads // kv_heads, kv_heads) + m_grad.shape[1:]).sum(axis=0)
        else:
            want = m_new
        assert_close(g_new, want, tol=2e-5, what=n)


@pytest.mark.parametrize('norm_first', [True, False])
def test_encoder_with_kv_heads_is_mha_with_repeated_kv_weights(npm, norm_first):
    rng = np.random.default_rng(8)
    b, s, f, heads, kv_heads = 2, 48, 128, 8, 2
    x = rng.standard_normal([b, s, f]).astype(np.float32)
    dy = rng.standard_normal([b, s, f]).astype(np.float32)
    gqa, mha = _pair(npm, npm.layers.TransformerEncoder, heads, kv_heads, 9, (x,), hidden_units=256, norm_first=norm_first)
    before = {n: np.asarray(getattr(gqa._self_attention, '_' + n)).copy() for n in _ATT}
    assert gqa._self_attention._wk.shape == (kv_heads, f // heads, f)
    assert_close(gqa(x), mha(x), tol=1e-5, what='out')
    lr = 0.01
    assert_close(gqa(dy, backprop=True, learning_rate=lr), mha(dy, backprop=True, learning_rate=lr), tol=1e-5, what='dx')
    _compare_attention_params(gqa._self_attention, mha._self_attention, before, heads, kv_heads, lr)


@pytest.mark.parametrize('norm_first', [True, False])
def test_decoder_with_kv_heads_is_mha_with_repeated_kv_weights(npm, norm_first):
    rng = np.random.default_rng(10)
    b, s, skv, f, heads, kv_heads = 2, 40, 56, 128, 8, 4
    q = rng.standard_normal([b, s, f]).astype(np.float32)
    kv = rng.standard_normal([b, skv, f]).astype(np.float32)
    dy = rng.standard_normal([b, s, f]).astype(np.float32)
    gqa, mha = _pair(npm, npm.layers.TransformerDecoder, heads, kv_heads, 12, (q, kv), hidden_units=256, norm_first=norm_first)
    before = {a: {n: np.asarray(getattr(getattr(gqa, a), '_' + n)).copy() for n in _ATT}
              for a in ('_self_attention', '_cross_attention')}
    assert gqa._cross_attention._wv.shape == (kv_heads, f // heads, f)
    assert_close(gqa(q, kv), mha(q, kv), tol=1e-5, what='out')
    lr = 0.01
    g_dq, g_dkv = gqa(dy, backprop=True, learning_rate=lr)
    m_dq, m_dkv = mha(dy, backprop=True, learning_rate=lr)
    assert_close(g_dq, m_dq, tol=1e-5, what='dq')
    assert_close(g_dkv, m_dkv, tol=1e-5, what='dkv')
    for a in ('_self_attention', '_cross_attention'):
        _compare_attention_params(getattr(gqa, a), getattr(mha, a), before[a], heads, kv_heads, lr)
