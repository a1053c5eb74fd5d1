"""Builders and checks shared by tests/test_rope_host.py (host simulator) and tests/test_gpu_rope.py (MI355X): layers with
``rope_base``, the comparison of npm_rope with tests/rope_reference.py ``rotate`` bit for bit, and the layer, decoding and
stored-row checks against the float64 reference.  A plain module like tests/decode_cases.py: every function takes ``npm``."""

import itertools

import numpy as np

import decode_cases as DC
import decode_gpu
import decode_reference as DR
import rope_reference as RR
import varlen_reference as VR
from conftest import assert_close

BASE = 1e4
LAYER_TOL = 1e-5                  # tests/test_gpu_decode.py: the bound of the cached-layer tests (float32 layer against float64)
GUARD, SENTINEL = decode_gpu.GUARD, decode_gpu.SENTINEL
EW_GRID_CAP_KNOB = 7              # include/npm_hip.h NPM_TUNE_EW_GRID_CAP: the grid cap npm_rope shares with the elementwise kernels


# ---- builders -----------------------------------------------------------------------------------------------------------------------
def make_mha(npm, features, heads, kv_heads, seed, batch=2, **kwargs):
    """tests/decode_cases.py ``make_mha`` with the layer's keywords: the same seed gives the same weights with and without
    ``rope_base`` (the tables are no parameters and draw nothing)."""
    np.random.seed(seed)
    att = npm.layers.MultiHeadAttention(heads, num_kv_heads=kv_heads, **kwargs)
    att(np.zeros([batch, 2, features], dtype=np.float32))
    for name in ('_wq', '_wk', '_wv', '_wo'):
        arr = getattr(att, name)
        arr.set(np.asarray(arr) * np.float32(2.0 / np.sqrt(features)))
    return att, {n: np.asarray(getattr(att, '_' + n)).astype(np.float64) for n in DC.ATT}


def _scale_weights(layer, paths, features):
    for path, attrs in paths:
        for attr in attrs:
            arr = getattr(DC.sub(layer, path), attr)
            arr.set(np.asarray(arr) * np.float32(2.0 / np.sqrt(features)))


_ATT_W = ('_wq', '_wk', '_wv', '_wo')


def make_decoder(npm, features, heads, kv_heads, hidden, norm_first, seed, batch=2, seq_kv=7, **kwargs):
    """A causal TransformerDecoder with O(1) activations (tests/decode_cases.py ``make_decoder``) and the layer's keywords."""
    np.random.seed(seed)
    dec = npm.layers.TransformerDecoder(num_heads=heads, hidden_units=hidden, norm_first=norm_first, num_kv_heads=kv_heads,
                                        causal=True, **kwargs)
    dec(np.zeros([batch, 2, features], dtype=np.float32), np.zeros([batch, seq_kv, features], dtype=np.float32))
    _scale_weights(dec, (('_self_attention', _ATT_W), ('_cross_attention', _ATT_W), ('_dense1._linear', ('_w',)), ('_dense2', ('_w',))),
                   features)
    return dec, DC.decoder_params(dec)


def make_encoder(npm, features, heads, kv_heads, hidden, norm_first, seed, batch=2, **kwargs):
    np.random.seed(seed)
    enc = npm.layers.TransformerEncoder(num_heads=heads, hidden_units=hidden, norm_first=norm_first, num_kv_heads=kv_heads, **kwargs)
    enc(np.zeros([batch, 2, features], dtype=np.float32))
    _scale_weights(enc, (('_self_attention', _ATT_W), ('_dense1._linear', ('_w',)), ('_dense2', ('_w',))), features)
    return enc, {k: np.asarray(getattr(DC.sub(enc, path), attr)).astype(np.float64) for k, (path, attr) in RR.ENC.items()}


def _grads(rec, layer, names):
    return {k: rec.grads[(id(DC.sub(layer, path)), attr)] for k, (path, attr) in names.items()}


# ---- the kernel, bit for bit --------------------------------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def run_rope(npm, x, heads, d, tables, at=0, at_lens=None, inverse=0, offset=0, table_rows=None, expect=0, twice=False, dev=None):
    """``x`` host float32 [B, T, pitch]: npm_rope on the first ``heads`` heads of every row through the C ABI, on a device buffer
    entered ``offset`` floats behind its start with a guard region behind it (``dev``: the tables, already on the device).
    Returns the rows afterwards."""
    from np_modeling_amd import _C, device as D
    b, t, pitch = x.shape
    cos, sin = dev if dev is not None else device_tables(npm, tables)
    rows = tables[0].shape[0] if table_rows is None else table_rows
    buf = D.full([offset + x.size + GUARD], SENTINEL)
    buf.flat_view(offset, [x.size]).set(x.ravel())
    lens = None if at_lens is None else decode_gpu.ints(at_lens)
    for _ in range(2 if twice else 1):
        rc = _C.lib().npm_rope(buf.ptr + 4 * offset, pitch, b, t, heads, d, cos.ptr, sin.ptr, rows, at, None if lens is None else lens.ptr,
                               inverse)
        assert rc == expect, (rc, _C.lib().npm_last_error())
    host = buf.numpy()
    assert (host[:offset] == SENTINEL).all() and (host[offset + x.size:] == SENTINEL).all(), 'a write outside the rows'
    return host[offset:offset + x.size].reshape(b, t, pitch)


def device_tables(npm, tables):
    return tuple(npm.device.from_host(tab) for tab in tables)


def expected_rows(x, heads, d, tables, at=0, at_lens=None, inverse=0, table_rows=None):
    """What npm_rope leaves: the bitwise model on the first ``heads`` heads of the rows whose position is inside the table,
    everything else as it was."""
    b, t, pitch = x.shape
    rows = tables[0].shape[0] if table_rows is None else table_rows
    start = np.full(b, at) if at_lens is None else np.asarray(at_lens)
    positions = start[:, None] + np.arange(t)[None, :]
    inside = (positions >= 0) & (positions < rows)
    want = x.copy()
    head_part = x[:, :, :heads * d].reshape(b, t, heads, d)
    rotated = RR.rotate(head_part, np.where(inside, positions, 0), tables[0], tables[1], inverse=bool(inverse)).reshape(b, t, heads * d)
    want[:, :, :heads * d][inside] = rotated[inside]
    return want


def kernel_rows(rng, b, t, heads, d, extra_heads):
    """N(0, 1) rows [B, T, (heads + extra_heads) * d] whose trailing heads (the V part of a packed projection) hold a sentinel."""
    x = np.full([b, t, (heads + extra_heads) * d], np.float32(-123.25))
    x[:, :, :heads * d] = rng.standard_normal([b, t, heads * d]).astype(np.float32)
    return x


VEC_DIMS, SCALAR_DIMS = (16, 32, 64, 128), (2, 6, 12, 20)
RAGGED_AT = (33, 0, 7)


def kernel_grid():
    """(d, heads, b, t, extra_heads, at, ragged, inverse): the full product of the axes."""
    return list(itertools.product(VEC_DIMS + SCALAR_DIMS, (1, 3, 10), ((1, 1), (3, 5), (2, 17)), (0, 4), (0, 35, 'ragged'), (0, 1)))


def check_kernel_case(npm, rng, tables, dev, d, heads, bt, extra_heads, at, inverse):
    b, t = bt
    x = kernel_rows(rng, b, t, heads, d, extra_heads)
    at_lens = list(RAGGED_AT[:b]) if at == 'ragged' else None
    at = 0 if at == 'ragged' else at
    got = run_rope(npm, x, heads, d, tables[d], at, at_lens, inverse, dev=dev[d])
    want = expected_rows(x, heads, d, tables[d], at, at_lens, inverse)
    assert np.array_equal(bits(got), bits(want)), (d, heads, bt, extra_heads, at, at_lens, inverse)
    assert not np.array_equal(bits(got[:, :, :heads * d]), bits(x[:, :, :heads * d])) or (at == 0 and at_lens is None and t == 1)


# ---- layers against the float64 reference -------------------------------------------------------------------------------------------
def check_layer(npm, f, heads, kv_heads, tol=1e-4, core=None, seed=9):
    """B 2, S 9 self-attention: output, input gradients and every parameter gradient."""
    att, p = make_mha(npm, f, heads, kv_heads, seed=seed, rope_base=BASE)
    rng = np.random.default_rng(7)
    x, dy = rng.standard_normal([2, 9, f]).astype(np.float32), rng.standard_normal([2, 9, f]).astype(np.float32)
    want, c = RR.att_fwd(p, BASE, x.astype(np.float64))
    plain, _ = DR.att_fwd(p, x.astype(np.float64))
    assert np.abs(want - plain).max() > 1e-2                              # the rotation matters
    out = np.asarray(att(x))
    assert att._packed and (core is None or att._core == core)
    assert_close(out, want, tol=tol, what='out')
    (want_dq, want_dk, want_dv), want_g = RR.att_bwd(p, c, dy.astype(np.float64))
    rec = DC.GradRecorder()
    dq, dk, dv = (np.asarray(g) for g in att(dy, backprop=True, optimizer_=rec))
    for got, ref, what in ((dq, want_dq, 'dq'), (dk, want_dk, 'dk'), (dv, want_dv, 'dv')):
        assert_close(got, ref, tol=tol, what=what)
    for name in DC.ATT:
        assert_close(rec.grads[(id(att), '_' + name)], want_g[name], tol=tol, what=name)


def check_cross(npm, tol=1e-4):
    """Separate query / key / value tensors with Sq 5 != Skv 9: each side is counted from position 0."""
    att, p = make_mha(npm, 64, 4, 2, seed=10, rope_base=BASE)
    rng = np.random.default_rng(8)
    q, k, v, dy = (rng.standard_normal([2, s, 64]).astype(np.float32) for s in (5, 9, 9, 5))
    want, c = RR.att_fwd(p, BASE, q.astype(np.float64), k.astype(np.float64), v.astype(np.float64))
    assert_close(np.asarray(att(q, k, v)), want, tol=tol, what='out')
    assert not att._packed
    (want_dq, want_dk, want_dv), want_g = RR.att_bwd(p, c, dy.astype(np.float64))
    rec = DC.GradRecorder()
    grads = [np.asarray(g) for g in att(dy, backprop=True, optimizer_=rec)]
    for got, ref, what in zip(grads, (want_dq, want_dk, want_dv), ('dq', 'dk', 'dv')):
        assert_close(got, ref, tol=tol, what=what)
    for name in DC.ATT:
        assert_close(rec.grads[(id(att), '_' + name)], want_g[name], tol=tol, what=name)


def check_decoder(npm, norm_first, tol=1e-4):
    """A causal decoder with ``rope_base``, B 2, S 8, F 64, H 4, hidden 128: output, (dq, dkv) and all 26 parameter gradients."""
    f, s = 64, 8
    dec, p = make_decoder(npm, f, 4, None, 128, norm_first, seed=11, rope_base=BASE)
    assert dec._self_attention._rope_base == BASE and dec._cross_attention._rope_base is None
    rng = np.random.default_rng(12)
    q, kv, dy = (rng.standard_normal(shape).astype(np.float32) for shape in ([2, s, f], [2, 7, f], [2, s, f]))
    want, c = RR.decoder_fwd(p, BASE, q.astype(np.float64), kv.astype(np.float64), norm_first, mask=DR.causal_mask(s))
    plain, _ = DR.decoder_fwd(p, q.astype(np.float64), kv.astype(np.float64), norm_first, mask=DR.causal_mask(s))
    assert np.abs(want - plain).max() > 1e-3
    (want_dq, want_dkv), want_g = RR.decoder_bwd(p, c, dy.astype(np.float64), norm_first)
    assert_close(np.asarray(dec(q, kv)), want, tol=tol, what='out')
    rec = DC.GradRecorder()
    dq, dkv = (np.asarray(g) for g in dec(dy, backprop=True, optimizer_=rec))
    assert_close(dq, want_dq, tol=tol, what='dq')
    assert_close(dkv, want_dkv, tol=tol, what='dkv')
    grads = rec.named(dec)
    assert len(grads) == 26
    for name, grad in grads.items():
        if name == 'ca_bk':                   # exactly zero in real arithmetic (rows of datt sum to 0; no rotation there): rounding noise
            assert np.abs(grad).max() < 1e-4 and np.abs(want_g[name]).max() < 1e-9
            continue
        assert_close(grad, want_g[name], tol=tol, what=name)


def check_encoder(npm, norm_first, tol=1e-4):
    f, s = 64, 8
    enc, p = make_encoder(npm, f, 4, None, 128, norm_first, seed=13, rope_base=BASE)
    rng = np.random.default_rng(14)
    x, dy = rng.standard_normal([2, s, f]).astype(np.float32), rng.standard_normal([2, s, f]).astype(np.float32)
    want, c = RR.encoder_fwd(p, BASE, x.astype(np.float64), norm_first)
    want_dx, want_g = RR.encoder_bwd(p, c, dy.astype(np.float64), norm_first)
    assert_close(np.asarray(enc(x)), want, tol=tol, what='out')
    rec = DC.GradRecorder()
    assert_close(np.asarray(enc(dy, backprop=True, optimizer_=rec)), want_dx, tol=tol, what='dx')
    grads = _grads(rec, enc, RR.ENC)
    assert len(grads) == 16
    for name, grad in grads.items():
        assert_close(grad, want_g[name], tol=tol, what=name)


# ---- decoding -----------------------------------------------------------------------------------------------------------------------
SEQ, CAPACITY = 13, 16
RAGGED_SCHEDULE = ([5, 3, 0], [1, 1, 1], [3, 0, 5], [1, 1, 1], [3, 4, 6])      # 13, 9 and 13 tokens; each rides along once at n = 0
CACHES = dict(contiguous={}, paged=dict(page_size=16), f16=dict(dtype='f16'))


def _stored_step(p, x, cache, before):
    """float64 attention of the chunk ``x`` (its rows already appended) over the rows AS STORED, queries rotated at ``before`` + t:
    what tests/test_gpu_kv16.py holds an fp16 cache to."""
    k, v = (np.asarray(r, dtype=np.float64) for r in cache.gather(cache.max_length))
    ctx, _ = DR.decode_attention(RR.project_q(p, BASE, x, before), k, v, cache.length, 1.0 / np.sqrt(p['wq'].shape[1]), True)
    return np.einsum('...abc,...dbc->...ad', ctx, p['wo']) + p['bo']


def check_chunked_attention(npm, kind):
    """``att(x, cache=cache)`` in the chunkings of tests/decode_cases.py equals the whole causal forward row for row."""
    att, p = make_mha(npm, 64, 4, 2, seed=11, batch=3, rope_base=BASE)
    rng = np.random.default_rng(9)
    if kind == 'ragged':
        total = VR.schedule_rows(RAGGED_SCHEDULE)
        x_rows = [rng.standard_normal([s, 64]).astype(np.float32) for s in total]
        alone = [RR.att_fwd(p, BASE, x[None].astype(np.float64), mask=DR.causal_mask(len(x)))[0][0] for x in x_rows]
        for kwargs in ({}, dict(page_size=16)):
            cache = att.make_cache(3, CAPACITY, **kwargs)
            outs = [np.asarray(att(x, cache=cache, new_lengths=n)) for x, n in VR.padded_calls(x_rows, RAGGED_SCHEDULE)]
            assert cache.lengths.tolist() == total.tolist() and all(np.isfinite(o).all() for o in outs)
            for i, (got, want) in enumerate(zip(VR.collect(outs, RAGGED_SCHEDULE, 3), alone)):
                decode_gpu.layer_close(got, want, LAYER_TOL, f'ragged {kwargs} sequence {i} against itself alone')
        return
    x = rng.standard_normal([3, SEQ, 64]).astype(np.float32)
    want, _ = RR.att_fwd(p, BASE, x.astype(np.float64), mask=DR.causal_mask(SEQ))
    whole = np.asarray(att(x, mask=DR.causal_mask(SEQ)))
    decode_gpu.layer_close(whole, want, LAYER_TOL, 'the whole causal forward')
    for sizes in DC.chunkings(SEQ):
        cache = att.make_cache(3, CAPACITY, **CACHES[kind])
        outs = []
        for piece in DC.split(x, sizes):
            before = cache.length
            outs.append(np.asarray(att(np.ascontiguousarray(piece), cache=cache)))
            if kind == 'f16':                  # an fp16 cache is attended to as stored: float64 over the stored (rotated, rounded) rows
                decode_gpu.layer_close(outs[-1], _stored_step(p, piece, cache, before), LAYER_TOL, f'f16 chunk at {before} of {sizes[:4]}')
        assert cache.length == SEQ
        if kind != 'f16':
            got = np.concatenate(outs, axis=1)
            decode_gpu.layer_close(got, want, LAYER_TOL, f'{kind} chunks {sizes[:4]} against float64')
            decode_gpu.layer_close(got, whole, 2 * LAYER_TOL, f'{kind} chunks {sizes[:4]} against the whole forward')


def check_chunked_decoder(npm, kind, norm_first=True):
    """``dec.decode`` in chunks equals ``dec.forward`` on the whole sequence row for row."""
    f = 64
    dec, p = make_decoder(npm, f, 4, 2, 128, norm_first, seed=15, batch=3, rope_base=BASE)
    rng = np.random.default_rng(16)
    kv = rng.standard_normal([3, 7, f]).astype(np.float32)
    if kind == 'ragged':
        total = VR.schedule_rows(RAGGED_SCHEDULE)
        q_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
        state = dec.start_decoding(kv, CAPACITY)
        outs = [np.asarray(dec.decode(x, state, new_lengths=n)) for x, n in VR.padded_calls(q_rows, RAGGED_SCHEDULE)]
        assert state.positions.tolist() == total.tolist()
        for i, got in enumerate(VR.collect(outs, RAGGED_SCHEDULE, 3)):
            want, _ = RR.decoder_fwd(p, BASE, q_rows[i][None].astype(np.float64), kv[i:i + 1].astype(np.float64), norm_first,
                                     mask=DR.causal_mask(len(q_rows[i])))
            decode_gpu.layer_close(got, want[0], 1e-4, f'ragged decode, sequence {i} against itself alone')
        return
    kwargs = dict(contiguous={}, paged=dict(page_size=16), f16=dict(cache_dtype='f16'))[kind]
    q = rng.standard_normal([3, SEQ, f]).astype(np.float32)
    want, _ = RR.decoder_fwd(p, BASE, q.astype(np.float64), kv.astype(np.float64), norm_first, mask=DR.causal_mask(SEQ))
    whole = np.asarray(dec(q, kv)) if kind != 'f16' else np.asarray(dec.decode(q, dec.start_decoding(kv, CAPACITY, **kwargs)))
    for sizes in DC.chunkings(SEQ):
        state = dec.start_decoding(kv, CAPACITY, **kwargs)
        got = np.concatenate([np.asarray(dec.decode(np.ascontiguousarray(piece), state)) for piece in DC.split(q, sizes)], axis=1)
        assert state.position == SEQ
        decode_gpu.layer_close(got, whole, 2 * LAYER_TOL, f'{kind} decode chunks {sizes[:4]} against one call')
        if kind != 'f16':
            decode_gpu.layer_close(got, want, 1e-4, f'{kind} decode chunks {sizes[:4]} against float64')


def check_release_and_admit(npm, norm_first=True):
    """A sequence admitted into a freed slot starts at position 0: it equals that sequence decoded alone."""
    f = 64
    dec, p = make_decoder(npm, f, 4, 2, 128, norm_first, seed=17, batch=2, rope_base=BASE)
    rng = np.random.default_rng(18)
    kv = rng.standard_normal([3, 7, f]).astype(np.float32)                # the memories of sequences 0, 1 and the admitted one
    rows = [rng.standard_normal([s, f]).astype(np.float32) for s in (9, 6, 5)]
    state = dec.start_decoding(kv[:2], CAPACITY, page_size=16)
    pad = lambda a, b: np.stack([np.concatenate([r, np.zeros([max(len(a), len(b)) - len(r), f], dtype=np.float32)]) for r in (a, b)])
    first = np.asarray(dec.decode(pad(rows[0][:5], rows[1][:5]), state))                       # both prompts
    second = np.asarray(dec.decode(pad(rows[0][5:6], rows[1][5:6]), state))
    state.release(1)
    dec.admit(state, 1, kv[2:3])
    assert state.positions.tolist() == [6, 0]
    third = np.asarray(dec.decode(pad(rows[0][6:7], rows[2][:4]), state, new_lengths=[1, 4]))   # the admitted prompt beside a token
    fourth = np.asarray(dec.decode(pad(rows[0][7:8], rows[2][4:5]), state))
    assert state.positions.tolist() == [8, 5]
    got = {0: np.concatenate([first[0], second[0], third[0, :1], fourth[0]]), 1: np.concatenate([first[1], second[1]]),
           2: np.concatenate([third[1, :4], fourth[1]])}
    for i, mem in ((0, 0), (1, 1), (2, 2)):
        n = len(got[i])
        want, _ = RR.decoder_fwd(p, BASE, rows[i][None, :n].astype(np.float64), kv[mem:mem + 1].astype(np.float64), norm_first,
                                 mask=DR.causal_mask(n))
        decode_gpu.layer_close(got[i], want[0], 1e-4, f'sequence {i} against itself alone from position 0')


def check_prefill_switch(npm, f16):
    """A 40-token chunk on 8 cached rows with the prefill kernel of that cache type switched on (the caller restores the switch)."""
    D = npm.device
    att, p = make_mha(npm, 64, 4, 2, seed=19, rope_base=BASE)
    x = np.random.default_rng(20).standard_normal([2, 48, 64]).astype(np.float32)
    setattr(D, 'PREFILL_KERNEL_F16' if f16 else 'PREFILL_KERNEL', True)
    cache = att.make_cache(2, 64, dtype='f16' if f16 else 'f32')
    att(np.ascontiguousarray(x[:, :8]), cache=cache)
    got = np.asarray(att(np.ascontiguousarray(x[:, 8:]), cache=cache))
    assert att._cached_path == 'prefill' and cache.length == 48
    if f16:
        want = _stored_step(p, x[:, 8:], cache, 8)
    else:
        want = RR.att_fwd(p, BASE, x.astype(np.float64), mask=DR.causal_mask(48))[0][:, 8:]
    decode_gpu.layer_close(got, want, LAYER_TOL, f'prefill kernel, f16={f16}')


# ---- the stored rows ----------------------------------------------------------------------------------------------------------------
def check_stored_rows(npm, kind, ragged):
    """Two layers with the same weights, one with ``rope_base``: after a prefill and two decode steps the rotating layer's cache
    holds, bit for bit, the bitwise model's rotation of the plain layer's K rows, and the same V rows."""
    rope, _ = make_mha(npm, 64, 4, 2, seed=21, rope_base=BASE)
    plain, _ = make_mha(npm, 64, 4, 2, seed=21)
    assert all(np.array_equal(np.asarray(getattr(rope, n)), np.asarray(getattr(plain, n))) for n in ('_wq', '_wk', '_wv', '_wo', '_bk'))
    rng = np.random.default_rng(22)
    x = rng.standard_normal([2, 5, 64]).astype(np.float32)
    steps = [(5, [5, 3]), (1, [1, 1]), (1, [1, 0])] if ragged else [(5, None), (1, None), (1, None)]
    cache_rope = rope.make_cache(2, CAPACITY, **CACHES[kind])
    cache_plain = plain.make_cache(2, CAPACITY, **(CACHES[kind] if kind != 'f16' else {}))
    for i, (t, n) in enumerate(steps):
        piece = np.ascontiguousarray(x[:, i:i + t] if t == 1 else x)
        rope(piece, cache=cache_rope, new_lengths=n)
        plain(piece, cache=cache_plain, new_lengths=n)
    lengths = cache_rope.lengths
    assert lengths.tolist() == cache_plain.lengths.tolist() == ([7, 4] if ragged else [7, 7])
    rows = int(lengths.max())
    (k_rope, v_rope), (k_plain, v_plain) = ([np.asarray(a) for a in c.gather(rows)] for c in (cache_rope, cache_plain))
    cos, sin = RR.tables(CAPACITY, 16, BASE)
    want_k, want_v = RR.rotate(k_plain, np.arange(rows)[None, :], cos, sin), v_plain
    if kind == 'f16':
        want_k, want_v = (a.astype(np.float16).astype(np.float32) for a in (want_k, want_v))
    valid = np.arange(rows)[None, :] < lengths[:, None]
    assert np.array_equal(bits(k_rope)[valid], bits(want_k)[valid]), 'K rows are not the rotation of the plain rows, bit for bit'
    assert np.array_equal(bits(v_rope)[valid], bits(want_v)[valid]), 'V rows differ'
    assert not np.array_equal(bits(k_rope)[:, 1:], bits(k_plain)[:, 1:])  # rotated at all (position 0 is the identity)


def check_off_switch(npm):
    """``rope_base=None``: output and gradients are, bit for bit, those of a layer constructed without the keyword."""
    results = []
    for kwargs in ({}, dict(rope_base=None)):
        att, _ = make_mha(npm, 64, 4, 2, seed=23, **kwargs)
        rng = np.random.default_rng(24)
        x, dy = rng.standard_normal([2, 9, 64]).astype(np.float32), rng.standard_normal([2, 9, 64]).astype(np.float32)
        rec = DC.GradRecorder()
        out = [np.asarray(att(x))] + [np.asarray(g) for g in att(dy, backprop=True, optimizer_=rec)]
        assert att._rope is None
        results.append(out + [rec.grads[(id(att), '_' + n)] for n in DC.ATT])
    for a, b in zip(*results):
        assert np.array_equal(a, b)
