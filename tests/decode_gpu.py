"""Drivers shared by the GPU tests of incremental decoding (tests/test_gpu_decode.py, tests/test_gpu_varlen.py,
tests/test_gpu_paged.py): guard regions and their sentinel, the tuning knobs, the layer comparison, and -- for the ragged and
the paged entry points, which are held to the same float64 reference at the same bounds -- one ``run`` through the C ABI and one
``check``.  A plain module like tests/decode_cases.py: no fixtures (each test file keeps its own ``npm`` and its autouse reset)."""

import ctypes as C

import numpy as np

import attn_range_data as R
import varlen_reference as VR

GUARD = 64
SENTINEL = 777.0
SPLITS_KNOB, NT_KNOB = 20, 21


def reset_knobs():
    from np_modeling_amd import _C
    for knob in (SPLITS_KNOB, NT_KNOB):
        _C.check(_C.lib().npm_set_tuning(knob, 0), 'npm_set_tuning')


def set_splits(mode, lmax):
    """Applies a split mode; returns the split count the call must report (None: automatic, read back through the ABI)."""
    from np_modeling_amd import _C
    tiles = (lmax + 15) // 16
    value = {'one': 1, 'auto': 0, 'many': min(tiles + 3, 1024)}.get(mode, mode)
    _C.check(_C.lib().npm_set_tuning(SPLITS_KNOB, int(value)), 'npm_set_tuning')
    return int(value) or None


def guarded(arr, n):
    np.testing.assert_array_equal(arr.flat_view(n, [arr.size - n]).numpy(), SENTINEL)
    return arr.flat_view(0, [n]).numpy()


def ints(values):
    from np_modeling_amd import device as D
    return D.bytes_from_host(np.ascontiguousarray(np.asarray(values, dtype=np.int32)))


def layer_close(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    frac = float((np.abs(got - want) / (tol * (np.abs(want) + max(np.abs(want).max(), 1.0)))).max())
    print(f'{what}: {frac:.3f} of {tol:.1e} (|ref| + max |ref|)')
    assert frac <= 1.0, f'{what}: {frac:.3g} of the bound {tol:.3g}'


def data(seed, b, t, hq, hkv, d, cap):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal([b, t, hq, d]).astype(np.float32), rng.standard_normal([b, cap, hkv, d]).astype(np.float32),
            rng.standard_normal([b, cap, hkv, d]).astype(np.float32))


def poison(q, k, v, kv_lens, new_lens, fill=np.nan):
    """Cache rows at and past each sequence's length, and the padded query rows, hold ``fill``."""
    k, v, q = k.copy(), v.copy(), q.copy()
    past = np.arange(k.shape[1])[None, :] >= np.asarray(kv_lens)[:, None]
    k[past], v[past] = fill, fill
    if new_lens is not None:
        q[np.arange(q.shape[1])[None, :] >= np.asarray(new_lens)[:, None]] = fill
    return q, k, v


def pad_rows(x, packed):
    """[..., rows, Hkv, D] -> [..., rows, Hkv * D (+ 4 floats of NaN padding)], and the row pitch."""
    hkv, d = x.shape[-2:]
    flat = x.reshape(x.shape[:-2] + (hkv * d,))
    if not packed:
        return np.ascontiguousarray(flat), hkv * d
    out = np.full(flat.shape[:-1] + (hkv * d + 4,), np.nan, dtype=np.float32)
    out[..., :hkv * d] = flat
    return out, hkv * d + 4


def run(q, k, v, lmax, scale, causal, kv_lens=None, new_lens=None, packed=False, paged=None, expect=0, null_lens=False,
        null_table=False):
    """q [B, T, Hq, D]; k / v [B, capacity, Hkv, D] (contiguous) or, with ``paged = (table [B, P], page_rows)``, page pools
    [pages, page_rows, Hkv, D] -> ctx, lse, kernel string.  ``paged``: npm_mha_decode_fwd_paged; else ``kv_lens`` None: the uniform
    entry point npm_mha_decode_fwd at kv_len = lmax; else (or with ``null_lens``: a NULL lengths pointer) npm_mha_decode_fwd_varlen
    with d->kv_len = lmax.  ``packed``: q sits in a [B, T, Hq + 2 Hkv, D] buffer and the cache rows carry 4 floats of padding (NaN
    in both).  ``expect``: the call must return that code and leave ctx untouched."""
    from np_modeling_amd import _C, device as D
    b, t, hq, d = q.shape
    rows, hkv = k.shape[1], k.shape[2]
    if packed:
        qp = hq * d + 2 * hkv * d
        qbuf = np.full([b, t, qp], np.nan, dtype=np.float32)
        qbuf[:, :, :hq * d] = q.reshape(b, t, hq * d)
    else:
        qp, qbuf = hq * d, q
    kbuf, kp = pad_rows(k, packed)
    vbuf, _ = pad_rows(v, packed)
    qd, kd, vd = D.from_host(qbuf), D.from_host(kbuf), D.from_host(vbuf)
    ctx = D.full([b * t * hq * d + GUARD], SENTINEL)
    lse = D.full([b * hq * t + GUARD], SENTINEL)
    c = _C.npm_mha_decode()
    c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim = b, hq, hkv, t, lmax, d
    c.causal, c.scale = int(causal), scale
    c.q, c.q_pitch = qd.ptr, qp
    c.k, c.k_pitch, c.k_stride_b = kd.ptr, kp, rows * kp
    c.v, c.v_pitch, c.v_stride_b = vd.ptr, kp, rows * kp
    c.ctx, c.ctx_pitch, c.lse = ctx.ptr, hq * d, lse.ptr
    lens = None if null_lens or kv_lens is None else ints(kv_lens)
    new = None if new_lens is None else ints(new_lens)
    lens_ptr, new_ptr = (None if x is None else x.ptr for x in (lens, new))
    if paged is not None:
        table, page_rows = paged
        assert table.min() >= 0 and table.max() < k.shape[0], 'every table entry must name a page of the pool'
        table_dev = ints(table)
        entry = 'npm_mha_decode_fwd_paged'
        rc = _C.lib().npm_mha_decode_fwd_paged(C.byref(c), lens_ptr, new_ptr, None if null_table else table_dev.ptr, table.shape[1],
                                               page_rows)
    elif kv_lens is None and not null_lens:
        entry = 'npm_mha_decode_fwd'
        rc = _C.lib().npm_mha_decode_fwd(C.byref(c))
    else:
        entry = 'npm_mha_decode_fwd_varlen'
        rc = _C.lib().npm_mha_decode_fwd_varlen(C.byref(c), lens_ptr, new_ptr)
    if expect:
        assert rc == expect, (rc, _C.lib().npm_last_error())
        assert (entry + ':').encode() in _C.lib().npm_last_error(), 'the error names the entry point that was called'
        np.testing.assert_array_equal(ctx.numpy(), SENTINEL)              # nothing was launched
        return None
    _C.check(rc, 'npm_mha_decode_fwd[_varlen|_paged]')
    return guarded(ctx, b * t * hq * d).reshape(b, t, hq, d), guarded(lse, b * hq * t).reshape(b, hq, t), _C.last_decode_kernel()


def check(got_ctx, got_lse, q, k, v, kv_lens, new_lens, scale, causal, what):
    """Every valid element against float64 of its sequence alone at tol(X) of that sequence; rows without a visible key are
    ctx == 0, lse == -inf.  Prints the largest fraction of the bound used."""
    b, t = q.shape[:2]
    want_ctx, want_lse = VR.decode_attention(q, k, v, kv_lens, new_lens, scale, causal)
    seen = VR.valid_rows(t, kv_lens, new_lens)
    assert (got_ctx[~seen] == 0).all(), f'{what}: ctx of a row without a visible key is not 0'
    assert np.isneginf(got_lse.transpose(0, 2, 1)[~seen]).all(), f'{what}: lse of a row without a visible key is not -inf'
    worst_ctx = worst_lse = 0.0
    for i in np.nonzero(seen.any(axis=1))[0]:
        rows = seen[i]
        g_ctx, g_lse = got_ctx[i, rows].astype(np.float64), got_lse[i][:, rows].astype(np.float64)
        assert np.isfinite(g_ctx).all() and np.isfinite(g_lse).all(), f'{what}: sequence {i} not finite'
        x = R.exponent_magnitude(q[i:i + 1, rows], k[i:i + 1, :kv_lens[i]], scale, want_lse[i:i + 1, :, rows])
        worst_ctx = max(worst_ctx, float((np.abs(g_ctx - want_ctx[i, rows]) / (R.exponent_tol(2e-6, x) * (1.0 + np.abs(want_ctx[i, rows])))).max()))
        worst_lse = max(worst_lse, float(np.abs(g_lse - want_lse[i][:, rows]).max() / R.exponent_tol(3e-6, x)))
    print(f'{what}: ctx {worst_ctx:.3f} of the bound, lse {worst_lse:.3f} of the bound')
    assert worst_ctx <= 1.0, f'{what}: ctx {worst_ctx:.3g} of the bound'
    assert worst_lse <= 1.0, f'{what}: lse {worst_lse:.3g} of the bound'
