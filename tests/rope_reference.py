"""NumPy restatement of rotary position embeddings (RoPE), shared by tests/test_rope_host.py and tests/test_gpu_rope.py.

Definition (include/npm_hip.h npm_rope).  D even, half = D / 2; element i < half of a head is paired with element i + half
("rotate-half"); the angle of position p and pair i is p * base ** (-i / half).
    forward   y[i] = x[i] c - x[i + half] s      y[i + half] = x[i + half] c + x[i] s
    inverse   y[i] = x[i] c + x[i + half] s      y[i + half] = x[i + half] c - x[i] s        (the transpose of the forward)

* ``tables``: cos / sin float32 [rows, half], computed in float64 and rounded once -- what the product uploads.
* ``rotate``: the BITWISE model of the kernel: float32 arrays, exactly the expressions above, so every product and every sum is
  rounded to float32 on its own (NumPy fuses nothing).
* ``rotate64``: float64 with exact angles (no table).
* ``att_fwd`` / ``att_bwd``: float64 attention with the rotation after the projections, on the conventions of
  tests/gqa_reference.py ``gqa_fwd`` / ``gqa_bwd`` (multi-head attention is its case Hkv == Hq); ``mha_cached``: the same layer
  fed in chunks with a growing cache, in the manner of tests/decode_reference.py; ``encoder_*`` / ``decoder_*``: the oracle's
  transformer layers with this self-attention.
"""

import numpy as np

import decode_reference as DR
import gqa_reference as G
from oracle import np_oracle as O


def inv_freq(d, base):
    half = d // 2
    return float(base) ** (-np.arange(half, dtype=np.float64) / half)


def tables(rows, d, base):
    """(cos, sin) float32 [rows, d / 2]; row p does not depend on ``rows``."""
    angle = np.arange(rows, dtype=np.float64)[:, None] * inv_freq(d, base)[None, :]
    return np.cos(angle).astype(np.float32), np.sin(angle).astype(np.float32)


def rotate(x, positions, cos, sin, inverse=False):
    """x float32 [..., H, D]; ``positions`` ints of shape x.shape[:-2] (or broadcastable to it).  Float32 throughout."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and cos.dtype == np.float32 and sin.dtype == np.float32
    half = x.shape[-1] // 2
    positions = np.broadcast_to(np.asarray(positions), x.shape[:-2])
    c, s = cos[positions][..., None, :], sin[positions][..., None, :]
    lo, hi = x[..., :half], x[..., half:]
    out = np.empty_like(x)
    if inverse:
        out[..., :half] = lo * c + hi * s
        out[..., half:] = hi * c - lo * s
    else:
        out[..., :half] = lo * c - hi * s
        out[..., half:] = hi * c + lo * s
    return out


def rotate64(x, positions, base, inverse=False):
    """The same in float64 with exact angles."""
    x = np.asarray(x, dtype=np.float64)
    half = x.shape[-1] // 2
    positions = np.broadcast_to(np.asarray(positions), x.shape[:-2])
    angle = positions[..., None].astype(np.float64) * inv_freq(x.shape[-1], base)
    c, s = np.cos(angle)[..., None, :], np.sin(angle)[..., None, :]
    if inverse:
        s = -s
    lo, hi = x[..., :half], x[..., half:]
    return np.concatenate([lo * c - hi * s, hi * c + lo * s], axis=-1)


# ---- attention with the rotation after the projections (float64) --------------------------------------------------------------
def att_fwd(p, base, query, key=None, value=None, mask=None, q_at=0, k_at=0):
    """tests/gqa_reference.py ``gqa_fwd`` with q rotated at positions q_at + 0 .. Sq - 1 and k at k_at + 0 .. Skv - 1.
    Returns (out, cache); the cache holds the ROTATED q and k."""
    key = query if key is None else key
    value = key if value is None else value
    wq, wk, wv, wo, bq, bk, bv, bo = (np.asarray(p[n], dtype=np.float64) for n in ('wq', 'wk', 'wv', 'wo', 'bq', 'bk', 'bv', 'bo'))
    query, key, value = (np.asarray(x, dtype=np.float64) for x in (query, key, value))
    num_q, key_dim = wq.shape[:2]
    num_kv, value_dim = wv.shape[:2]
    batch, seq_len_q = query.shape[:2]
    seq_len_kv = key.shape[1]
    pos_q, pos_k = q_at + np.arange(seq_len_q)[None, :], k_at + np.arange(seq_len_kv)[None, :]
    q = rotate64(np.einsum('...ab,cdb->...acd', query, wq) + bq, pos_q, base)
    k = rotate64(np.einsum('...ab,cdb->...acd', key, wk) + bk, pos_k, base)
    v = np.einsum('...ab,cdb->...acd', value, wv) + bv
    q5 = np.reshape(q, [batch, seq_len_q, num_q // num_kv, num_kv, key_dim])
    attention = np.einsum('...abcd,...ecd->...bcae', q5, k)
    attention = np.reshape(attention, [batch, num_q, seq_len_q, seq_len_kv]) * (1 / np.sqrt(key_dim))
    if mask is not None:
        attention = np.where(np.broadcast_to(mask, attention.shape), attention, float('-inf'))
    scores = G._softmax(attention)
    s5 = np.reshape(scores, [batch, num_q // num_kv, num_kv, seq_len_q, seq_len_kv])
    values = np.reshape(np.einsum('...abcd,...dbe->...cabe', s5, v), [batch, seq_len_q, num_q, value_dim])
    o = np.einsum('...abc,...dbc->...ad', values, wo) + bo
    cache = dict(query=query, key=key, value=value, q=q, k=k, v=v, scores=scores, values=values, mask=mask, rope_base=base,
                 pos_q=pos_q, pos_k=pos_k)
    return o, cache


def att_bwd(p, cache, dy):
    """tests/gqa_reference.py ``gqa_bwd`` with the inverse rotation on dq / dk in front of the in-projection gradients."""
    wq, wk, wv, wo = (np.asarray(p[n], dtype=np.float64) for n in ('wq', 'wk', 'wv', 'wo'))
    dy = np.asarray(dy, dtype=np.float64)
    query, key, value = cache['query'], cache['key'], cache['value']
    q, k, v, scores, values = cache['q'], cache['k'], cache['v'], cache['scores'], cache['values']
    num_q, key_dim = wq.shape[:2]
    num_kv = wk.shape[0]
    heads = np.arange(num_q) % num_kv
    kf, vf = k[:, :, heads], v[:, :, heads]
    g = {'bo': dy.sum(axis=(0, 1)), 'wo': np.einsum('bid,bihe->dhe', dy, values)}
    dvalues = np.einsum('bid,dhe->bihe', dy, wo)
    dscores = np.einsum('bihe,bjhe->bhij', dvalues, vf)
    dvf = np.einsum('bhij,bihe->bjhe', scores, dvalues)
    datt = scores * (dscores - np.sum(dscores * scores, axis=-1, keepdims=True)) / np.sqrt(key_dim)
    dq = np.einsum('bhij,bjhd->bihd', datt, kf)
    dkf = np.einsum('bhij,bihd->bjhd', datt, q)
    dk, dv = G.group_sum(dkf, num_kv), G.group_sum(dvf, num_kv)
    dq = rotate64(dq, cache['pos_q'], cache['rope_base'], inverse=True)
    dk = rotate64(dk, cache['pos_k'], cache['rope_base'], inverse=True)
    g['wq'] = np.einsum('bihd,bif->hdf', dq, query)
    g['wk'] = np.einsum('bjhd,bjf->hdf', dk, key)
    g['wv'] = np.einsum('bjhd,bjf->hdf', dv, value)
    g['bq'], g['bk'], g['bv'] = dq.sum(axis=(0, 1)), dk.sum(axis=(0, 1)), dv.sum(axis=(0, 1))
    dquery = np.einsum('bihd,hdf->bif', dq, wq)
    dkey = np.einsum('bjhd,hdf->bjf', dk, wk)
    dvalue = np.einsum('bjhd,hdf->bjf', dv, wv)
    return (dquery, dkey, dvalue), g


def project_q(p, base, x, at):
    """The rotated float64 queries [B, T, Hq, D] of a chunk whose sequence b starts at position at[b] (an int or [B])."""
    q = DR._project(np.asarray(x, dtype=np.float64), p['wq'], p['bq'])
    return rotate64(q, np.asarray(at).reshape(-1, 1) + np.arange(q.shape[1])[None, :], base)


def mha_cached(p, base, chunks, cache=None):
    """tests/decode_reference.py ``mha_cached`` with the rotation: every chunk's q and k are rotated at the positions behind the
    rows already in ``cache`` and the ROTATED k is what the cache keeps."""
    cache = {} if cache is None else cache
    scale = 1.0 / np.sqrt(p['wq'].shape[1])
    outs = []
    for x in chunks:
        x = np.asarray(x, dtype=np.float64)
        at = cache['k'].shape[1] if 'k' in cache else 0
        pos = at + np.arange(x.shape[1])[None, :]
        q = rotate64(DR._project(x, p['wq'], p['bq']), pos, base)
        k = rotate64(DR._project(x, p['wk'], p['bk']), pos, base)
        v = DR._project(x, p['wv'], p['bv'])
        cache['k'] = k if 'k' not in cache else np.concatenate([cache['k'], k], axis=1)
        cache['v'] = v if 'v' not in cache else np.concatenate([cache['v'], v], axis=1)
        ctx, _ = DR.decode_attention(q, cache['k'], cache['v'], cache['k'].shape[1], scale, True)
        outs.append(np.einsum('...abc,...dbc->...ad', ctx, p['wo']) + p['bo'])
    return np.concatenate(outs, axis=1)


# ---- the transformer layers with this self-attention ------------------------------------------------------------------------------
class _rotating_self_attention:
    """While active, tests/decode_reference.py's ``att_fwd`` / ``att_bwd`` rotate in every SELF-attention (a call without a key);
    a cross-attention stays what it is.  ``decoder_fwd`` / ``decoder_bwd`` there are then the decoder with ``rope_base``."""

    def __init__(self, base):
        self.base = base

    def __enter__(self):
        self.saved = DR.att_fwd, DR.att_bwd
        plain_fwd, plain_bwd, base = DR.att_fwd, DR.att_bwd, self.base
        DR.att_fwd = lambda p, query, key=None, value=None, mask=None: \
            att_fwd(p, base, query, mask=mask) if key is None else plain_fwd(p, query, key, value, mask)
        DR.att_bwd = lambda p, cache, dy: att_bwd(p, cache, dy) if 'rope_base' in cache else plain_bwd(p, cache, dy)

    def __exit__(self, *exc):
        DR.att_fwd, DR.att_bwd = self.saved
        return False


def decoder_fwd(p, base, q, kv, norm_first, mask=None):
    with _rotating_self_attention(base):
        return DR.decoder_fwd(p, q, kv, norm_first, mask)


def decoder_bwd(p, c, dy, norm_first):
    with _rotating_self_attention(None):
        return DR.decoder_bwd(p, c, dy, norm_first)


def encoder_fwd(p, base, qkv, norm_first, eps=1e-3):
    """oracle/np_oracle.py ``encoder_fwd`` (no dropout) from the oracle's own pieces, with the rotating self-attention."""
    b, s, f = qkv.shape
    c = {}
    skip = h = qkv
    if norm_first:
        c['n1_x'] = h
        h, c['n1'] = O.layernorm_fwd(h, p['n1_gamma'], p['n1_beta'], eps)
    out, c['att'] = att_fwd(O._att_params(p), base, h)
    out = out + skip
    if not norm_first:
        c['n1_x'] = out
        out, c['n1'] = O.layernorm_fwd(out, p['n1_gamma'], p['n1_beta'], eps)
    out = out.reshape(-1, f)
    skip = out
    if norm_first:
        c['n2_x'] = out
        out, c['n2'] = O.layernorm_fwd(out, p['n2_gamma'], p['n2_beta'], eps)
    c['d1_x'] = out
    out, c['d1_pre'] = O.dense_fwd(out, p['d1_w'], p['d1_b'])
    c['d2_x'] = out
    out = O.linear_fwd(out, p['d2_w'], p['d2_b']) + skip
    if not norm_first:
        c['n2_x'] = out
        out, c['n2'] = O.layernorm_fwd(out, p['n2_gamma'], p['n2_beta'], eps)
    return out.reshape(b, s, f), c


def encoder_bwd(p, c, dy, norm_first, eps=1e-3):
    b, s, f = dy.shape
    g = {}
    dy = dy.reshape(-1, f)
    if not norm_first:
        dy, g['n2_gamma'], g['n2_beta'] = O.layernorm_bwd(c['n2_x'], p['n2_gamma'], eps, c['n2'], dy)
    dskip = dy
    dy, g['d2_w'], g['d2_b'] = O.linear_bwd(c['d2_x'], p['d2_w'], dy)
    dy, g['d1_w'], g['d1_b'] = O.dense_bwd(c['d1_x'], p['d1_w'], c['d1_pre'], dy)
    if norm_first:
        dy, g['n2_gamma'], g['n2_beta'] = O.layernorm_bwd(c['n2_x'], p['n2_gamma'], eps, c['n2'], dy)
    dy = (dy + dskip).reshape(b, s, f)
    if not norm_first:
        dy, g['n1_gamma'], g['n1_beta'] = O.layernorm_bwd(c['n1_x'], p['n1_gamma'], eps, c['n1'], dy)
    dskip = dy
    (dq, dk, dv), ga = att_bwd(O._att_params(p), c['att'], dy)
    g.update({f'att_{n}': a for n, a in ga.items()})
    dy = dq + dk + dv
    if norm_first:
        dy, g['n1_gamma'], g['n1_beta'] = O.layernorm_bwd(c['n1_x'], p['n1_gamma'], eps, c['n1'], dy)
    return dy + dskip, g


ENC = dict(n1_gamma=('_norm1', '_gamma'), n1_beta=('_norm1', '_beta'), n2_gamma=('_norm2', '_gamma'), n2_beta=('_norm2', '_beta'),
           d1_w=('_dense1._linear', '_w'), d1_b=('_dense1._linear', '_b'), d2_w=('_dense2', '_w'), d2_b=('_dense2', '_b'))
for _n in ('wq', 'wk', 'wv', 'wo', 'bq', 'bk', 'bv', 'bo'):
    ENC['att_' + _n] = ('_self_attention', '_' + _n)
