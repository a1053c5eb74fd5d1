"""Float64 NumPy restatement of grouped-query attention: the reference's ``gqa_fwd`` (layers/attentions_test.py:282-333)
and a hand-derived backward.  Shared by tests/test_gqa_host.py and tests/test_gpu_gqa.py.

Shapes (Hq query heads, Hkv key / value heads, Dk = F / Hq, Dv = Fv / Hq):
    wq [Hq, Dk, F]   wk [Hkv, Dk, F]   wv [Hkv, Dv, Fv]   wo [F, Hq, Dv]
    bq [Hq, Dk]      bk [Hkv, Dk]      bv [Hkv, Dv]       bo [F]
Query head h = g * Hkv + c reads key / value head c = h % Hkv: the reference reshapes q to [B, Sq, Hq / Hkv, Hkv, Dk] and
contracts its Hkv axis with k's head axis (attentions_test.py:305-308, 323-326).
"""

import numpy as np


def _softmax(x):
    m = np.max(x, axis=-1, keepdims=True)
    e = np.exp(x - m)
    return e / np.sum(e, axis=-1, keepdims=True)


def gqa_fwd(p, query, key=None, value=None, mask=None):
    """attentions_test.py:282-333 with the reference's own einsums; ``mask`` (broadcast to [B, Hq, Sq, Skv]) applied as
    np.where(mask, attention, -inf) (attentions_test.py:312-313).  Returns (out, cache)."""
    key = query if key is None else key
    value = key if value is None else value
    wq, wk, wv, wo, bq, bk, bv, bo = (np.asarray(p[n], dtype=np.float64) for n in ('wq', 'wk', 'wv', 'wo', 'bq', 'bk', 'bv', 'bo'))
    query, key, value = (np.asarray(x, dtype=np.float64) for x in (query, key, value))
    num_q, key_dim = wq.shape[:2]
    num_kv, value_dim = wv.shape[:2]
    batch, seq_len_q = query.shape[:2]
    seq_len_kv = key.shape[1]
    q = np.einsum('...ab,cdb->...acd', query, wq) + bq
    k = np.einsum('...ab,cdb->...acd', key, wk) + bk
    v = np.einsum('...ab,cdb->...acd', value, wv) + bv
    q5 = np.reshape(q, [batch, seq_len_q, num_q // num_kv, num_kv, key_dim])
    attention = np.einsum('...abcd,...ecd->...bcae', q5, k)
    attention = np.reshape(attention, [batch, num_q, seq_len_q, seq_len_kv])
    attention = attention * (1 / np.sqrt(key_dim))
    if mask is not None:
        attention = np.where(np.broadcast_to(mask, attention.shape), attention, float('-inf'))
    with np.errstate(invalid='ignore'):
        scores = _softmax(attention)
    s5 = np.reshape(scores, [batch, num_q // num_kv, num_kv, seq_len_q, seq_len_kv])
    values = np.einsum('...abcd,...dbe->...cabe', s5, v)
    values = np.reshape(values, [batch, seq_len_q, num_q, value_dim])
    o = np.einsum('...abc,...dbc->...ad', values, wo) + bo
    cache = dict(query=query, key=key, value=value, q=q, k=k, v=v, scores=scores, values=values, mask=mask)
    return o, cache


def gqa_bwd(p, cache, dy):
    """Gradient of ``gqa_fwd``.  Returns ((dquery, dkey, dvalue), grads keyed like the params).  Each K / V head's gradient is
    the sum over the Hq / Hkv query heads that read it."""
    wq, wk, wv, wo = (np.asarray(p[n], dtype=np.float64) for n in ('wq', 'wk', 'wv', 'wo'))
    dy = np.asarray(dy, dtype=np.float64)
    query, key, value = cache['query'], cache['key'], cache['value']
    q, k, v, scores, values = cache['q'], cache['k'], cache['v'], cache['scores'], cache['values']
    num_q, key_dim = wq.shape[:2]
    num_kv = wk.shape[0]
    heads = np.arange(num_q) % num_kv                  # the K / V head of each query head
    kf, vf = k[:, :, heads], v[:, :, heads]            # [B, Skv, Hq, D]
    g = {'bo': dy.sum(axis=(0, 1)), 'wo': np.einsum('bid,bihe->dhe', dy, values)}
    dvalues = np.einsum('bid,dhe->bihe', dy, wo)                       # [B, Sq, Hq, Dv]
    dscores = np.einsum('bihe,bjhe->bhij', dvalues, vf)
    dvf = np.einsum('bhij,bihe->bjhe', scores, dvalues)
    datt = scores * (dscores - np.sum(dscores * scores, axis=-1, keepdims=True)) / np.sqrt(key_dim)
    dq = np.einsum('bhij,bjhd->bihd', datt, kf)
    dkf = np.einsum('bhij,bihd->bjhd', datt, q)
    dk, dv = group_sum(dkf, num_kv), group_sum(dvf, num_kv)
    g['wq'] = np.einsum('bihd,bif->hdf', dq, query)
    g['wk'] = np.einsum('bjhd,bjf->hdf', dk, key)
    g['wv'] = np.einsum('bjhd,bjf->hdf', dv, value)
    g['bq'], g['bk'], g['bv'] = dq.sum(axis=(0, 1)), dk.sum(axis=(0, 1)), dv.sum(axis=(0, 1))
    dquery = np.einsum('bihd,hdf->bif', dq, wq)
    dkey = np.einsum('bjhd,hdf->bjf', dk, wk)
    dvalue = np.einsum('bjhd,hdf->bjf', dv, wv)
    return (dquery, dkey, dvalue), g


def group_sum(x, num_kv: int):
    """[..., Hq, D] per query head -> [..., Hkv, D]: out[..., c, :] = sum over g of x[..., g * Hkv + c, :]."""
    shape = x.shape
    return x.reshape(shape[:-2] + (shape[-2] // num_kv, num_kv, shape[-1])).sum(axis=-3)


def expand_kv(x, num_q: int):
    """[..., Hkv, ...] K / V heads on axis ``-2`` -> one per query head (head h % Hkv)."""
    return np.take(x, np.arange(num_q) % x.shape[-2], axis=-2)


def init_params(rng, f: int, fv: int, num_q: int, num_kv: int, scale: float = 1.0):
    """Parameters of the shapes above in the reference MHA's draw order wq, wk, wv, wo, bq, bk, bv, bo."""
    dk, dv = f // num_q, fv // num_q
    shapes = dict(wq=[num_q, dk, f], wk=[num_kv, dk, f], wv=[num_kv, dv, fv], wo=[f, num_q, dv],
                  bq=[num_q, dk], bk=[num_kv, dk], bv=[num_kv, dv], bo=[f])
    return {n: rng.standard_normal(s) * (scale if n.startswith('w') else 1.0) for n, s in shapes.items()}
