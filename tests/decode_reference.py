"""Float64 NumPy restatement of incremental decoding, shared by tests/test_decode_host.py and tests/test_gpu_decode.py.

* ``decode_attention``: attention of T new query tokens over the first L rows of a key / value cache -- the definition in
  include/npm_hip.h (npm_mha_decode_fwd) -- through the float64 reference of tests/attn_range_data.py with the causal rule
  written as a mask.
* ``split_model``: a float32 model of the kernel's split / combine rule: every split of the keys leaves (m, l, acc[D]) per row
  (m in log2 units), the splits are merged in split order, a split without a visible key has m = -inf, l = 0 and gets weight 0.
* ``auto_splits``: the automatic split count (csrc/npm_decode.hip npm_mha_decode_splits), restated.
* ``causal_mask`` / ``decoder_fwd`` / ``decoder_bwd``: the reference's TransformerDecoder (layers/transformer.py:117-203) with a
  mask on the self-attention.  oracle/np_oracle.py's decoder_fwd takes none, so the composition is restated here from the
  oracle's own functions (O.mha_fwd / O.mha_bwd take a mask; O.layernorm_*, O.linear_*, O.dense_*); with an all-true mask it is
  O.decoder_fwd / O.decoder_bwd exactly (tests/test_decode_host.py).  Grouped-query attention goes through tests/gqa_reference.py.
* ``mha_cached`` / ``decoder_cached``: the same layers fed in chunks with a key / value cache.
"""

import numpy as np

import attn_range_data as R
import gqa_reference as G
from oracle import np_oracle as O

TILE = 16                 # keys per tile of mha_decode_kernel: splits are ranges of whole tiles


def causal_rows(tokens, length):
    """[T, L] bool: new token t (the last T keys of the cache are the new tokens) sees keys j <= L - T + t."""
    return np.arange(length)[None, :] <= (length - tokens + np.arange(tokens))[:, None]


def causal_mask(seq):
    return np.tril(np.ones([seq, seq], dtype=bool))


def decode_attention(q, k, v, length, scale, causal):
    """q [B, T, Hq, D], k / v [B, capacity, Hkv, D] -> ctx [B, T, Hq, D], lse [B, Hq, T] in float64 over rows 0 .. length - 1."""
    tokens = q.shape[1]
    mask = causal_rows(tokens, length)[None, None] if causal else None
    out = R.reference(q, k[:, :length], v[:, :length], None, scale, mask=mask, grads=False)
    return out['ctx'], out['lse']


def auto_splits(batch, kv_heads, length):
    planes = batch * kv_heads
    return max(1, min((512 + planes - 1) // planes, max(1, length // 256), 1024))


def split_ranges(length, splits):
    tiles = (length + TILE - 1) // TILE
    per = (tiles + splits - 1) // splits
    return [(min(s * per * TILE, length), min((s + 1) * per * TILE, length)) for s in range(splits)]


def split_model(q, k, v, length, scale, causal, splits):
    """The split / combine rule in float32 (one (batch, K / V head) group at a time).  Returns ctx, lse as float32."""
    f = np.float32
    b, tokens, hq, d = q.shape
    hkv = k.shape[2]
    c2 = f(f(scale) * f(R.LOG2E))
    visible = causal_rows(tokens, length) if causal else np.ones([tokens, length], dtype=bool)
    ctx = np.zeros([b, tokens, hq, d], dtype=f)
    lse = np.zeros([b, hq, tokens], dtype=f)
    for bi in range(b):
        for h in range(hq):
            kp, vp = k[bi, :length, h % hkv].astype(f), v[bi, :length, h % hkv].astype(f)
            x = np.where(visible, (q[bi, :, h].astype(f) @ kp.T) * c2, f(-np.inf)).astype(f)       # [T, L], log2 units
            parts = []
            for lo, hi in split_ranges(length, splits):
                xs = x[:, lo:hi]
                m = xs.max(axis=1) if hi > lo else np.full(tokens, -np.inf, dtype=f)
                ref = np.where(np.isneginf(m), f(0), m).astype(f)
                p = np.exp2(xs - ref[:, None]).astype(f)
                parts.append((m.astype(f), p.sum(axis=1, dtype=f), (p @ vp[lo:hi]).astype(f)))
            top = np.max([m for m, _, _ in parts], axis=0)
            tot, acc = np.zeros(tokens, dtype=f), np.zeros([tokens, d], dtype=f)
            for m, l, a in parts:                                         # split order
                w = np.where(np.isneginf(m), f(0), np.exp2(np.where(np.isneginf(m), f(0), m - top))).astype(f)
                tot = (tot + l * w).astype(f)
                acc = (acc + a * w[:, None]).astype(f)
            ctx[bi, :, h] = acc / tot[:, None]
            lse[bi, h] = (top + np.log2(tot)).astype(f) * f(0.6931471805599453)
    return ctx, lse


# ---- attention layer and decoder with a mask on the self-attention ----------------------------------------------------------
def _grouped(p):
    return p['wk'].shape[0] != p['wq'].shape[0]


def att_fwd(p, query, key=None, value=None, mask=None):
    """The oracle's MHA, or tests/gqa_reference.py when the parameters have fewer K / V heads.  (out, cache)."""
    if _grouped(p):
        return G.gqa_fwd(p, query, key, value, mask)
    with np.errstate(invalid='ignore'):
        return O.mha_fwd(p, query, key, value, mask=mask)


def att_bwd(p, cache, dy):
    return G.gqa_bwd(p, cache, dy) if _grouped(p) else O.mha_bwd(p, cache, dy)


def decoder_fwd(p, q, kv, norm_first, mask=None, eps=1e-3):
    """O.decoder_fwd (no dropout) with ``mask`` on the self-attention."""
    b, s, f = q.shape
    c = {}
    skip = h = q
    if norm_first:
        c['n1_x'] = h
        h, c['n1'] = O.layernorm_fwd(h, p['n1_gamma'], p['n1_beta'], eps)
    out, c['sa'] = att_fwd(O._att(p, 'sa'), h, mask=mask)
    out = out + skip
    if not norm_first:
        c['n1_x'] = out
        out, c['n1'] = O.layernorm_fwd(out, p['n1_gamma'], p['n1_beta'], eps)
    skip = out
    if norm_first:
        c['n2_x'] = out
        out, c['n2'] = O.layernorm_fwd(out, p['n2_gamma'], p['n2_beta'], eps)
    out, c['ca'] = att_fwd(O._att(p, 'ca'), out, kv)
    out = out + skip
    if not norm_first:
        c['n2_x'] = out
        out, c['n2'] = O.layernorm_fwd(out, p['n2_gamma'], p['n2_beta'], eps)
    out = out.reshape(-1, f)
    skip = out
    if norm_first:
        c['n3_x'] = out
        out, c['n3'] = O.layernorm_fwd(out, p['n3_gamma'], p['n3_beta'], eps)
    c['d1_x'] = out
    out, c['d1_pre'] = O.dense_fwd(out, p['d1_w'], p['d1_b'])
    c['d2_x'] = out
    out = O.linear_fwd(out, p['d2_w'], p['d2_b']) + skip
    if not norm_first:
        c['n3_x'] = out
        out, c['n3'] = O.layernorm_fwd(out, p['n3_gamma'], p['n3_beta'], eps)
    return out.reshape(b, s, f), c


def decoder_bwd(p, c, dy, norm_first, eps=1e-3):
    """O.decoder_bwd (no dropout) for ``decoder_fwd`` above: ((dq, dkv), grads)."""
    b, s, f = dy.shape
    g = {}
    dy = dy.reshape(-1, f)
    if not norm_first:
        dy, g['n3_gamma'], g['n3_beta'] = O.layernorm_bwd(c['n3_x'], p['n3_gamma'], eps, c['n3'], dy)
    dskip = dy
    dy, g['d2_w'], g['d2_b'] = O.linear_bwd(c['d2_x'], p['d2_w'], dy)
    dy, g['d1_w'], g['d1_b'] = O.dense_bwd(c['d1_x'], p['d1_w'], c['d1_pre'], dy)
    if norm_first:
        dy, g['n3_gamma'], g['n3_beta'] = O.layernorm_bwd(c['n3_x'], p['n3_gamma'], eps, c['n3'], dy)
    dy = (dy + dskip).reshape(b, s, f)
    if not norm_first:
        dy, g['n2_gamma'], g['n2_beta'] = O.layernorm_bwd(c['n2_x'], p['n2_gamma'], eps, c['n2'], dy)
    dskip = dy
    (dq, dk, dv), ga = att_bwd(O._att(p, 'ca'), c['ca'], dy)
    g.update({f'ca_{n}': a for n, a in ga.items()})
    dkv = dk + dv
    dy = dq
    if norm_first:
        dy, g['n2_gamma'], g['n2_beta'] = O.layernorm_bwd(c['n2_x'], p['n2_gamma'], eps, c['n2'], dy)
    dy = dy + dskip
    if not norm_first:
        dy, g['n1_gamma'], g['n1_beta'] = O.layernorm_bwd(c['n1_x'], p['n1_gamma'], eps, c['n1'], dy)
    dskip = dy
    (dq, dk, dv), ga = att_bwd(O._att(p, 'sa'), c['sa'], dy)
    g.update({f'sa_{n}': a for n, a in ga.items()})
    dy = dq + dk + dv
    if norm_first:
        dy, g['n1_gamma'], g['n1_beta'] = O.layernorm_bwd(c['n1_x'], p['n1_gamma'], eps, c['n1'], dy)
    return (dy + dskip, dkv), g


# ---- the same layers, fed in chunks with a cache ---------------------------------------------------------------------------
def _project(x, w, bias):
    return np.einsum('...ab,cdb->...acd', x, w) + bias


def mha_cached(p, chunks, cache=None):
    """Self-attention over a sequence fed in ``chunks`` ([B, T_i, F] each): K / V of every chunk are appended to ``cache``
    (a dict k, v of [B, n, Hkv, D], grown here) and the chunk attends causally to all of it.  Returns the outputs, concatenated."""
    cache = {} if cache is None else cache
    scale = 1.0 / np.sqrt(p['wq'].shape[1])
    outs = []
    for x in chunks:
        x = np.asarray(x, dtype=np.float64)
        q, k, v = _project(x, p['wq'], p['bq']), _project(x, p['wk'], p['bk']), _project(x, p['wv'], p['bv'])
        cache['k'] = k if 'k' not in cache else np.concatenate([cache['k'], k], axis=1)
        cache['v'] = v if 'v' not in cache else np.concatenate([cache['v'], v], axis=1)
        ctx, _ = decode_attention(q, cache['k'], cache['v'], cache['k'].shape[1], scale, True)
        outs.append(np.einsum('...abc,...dbc->...ad', ctx, p['wo']) + p['bo'])
    return np.concatenate(outs, axis=1)


def mha_cross_cached(p, x, kv_cache):
    """Cross-attention of ``x`` over a filled, frozen cache (dict k, v): every key visible."""
    q = _project(np.asarray(x, dtype=np.float64), p['wq'], p['bq'])
    ctx, _ = decode_attention(q, kv_cache['k'], kv_cache['v'], kv_cache['k'].shape[1], 1.0 / np.sqrt(p['wq'].shape[1]), False)
    return np.einsum('...abc,...dbc->...ad', ctx, p['wo']) + p['bo']


def decoder_cached(p, chunks, kv, norm_first, eps=1e-3):
    """The decoder step by step: each chunk through cached causal self-attention, cross-attention over the K / V of ``kv``
    projected once, feed-forward and the three norms.  Returns the outputs, concatenated."""
    sa, ca = O._att(p, 'sa'), O._att(p, 'ca')
    kv = np.asarray(kv, dtype=np.float64)
    cross = dict(k=_project(kv, ca['wk'], ca['bk']), v=_project(kv, ca['wv'], ca['bv']))
    self_cache = {}
    norm = lambda x, n: O.layernorm_fwd(x, p[f'{n}_gamma'], p[f'{n}_beta'], eps)[0]
    outs = []
    for q in chunks:
        q = np.asarray(q, dtype=np.float64)
        b, t, f = q.shape
        h = norm(q, 'n1') if norm_first else q
        out = mha_cached(sa, [h], self_cache) + q
        if not norm_first:
            out = norm(out, 'n1')
        skip = out
        h = norm(out, 'n2') if norm_first else out
        out = mha_cross_cached(ca, h, cross) + skip
        if not norm_first:
            out = norm(out, 'n2')
        out = out.reshape(-1, f)
        skip = out
        h = norm(out, 'n3') if norm_first else out
        h, _ = O.dense_fwd(h, p['d1_w'], p['d1_b'])
        out = O.linear_fwd(h, p['d2_w'], p['d2_b']) + skip
        if not norm_first:
            out = norm(out, 'n3')
        outs.append(out.reshape(b, t, f))
    return np.concatenate(outs, axis=1)
