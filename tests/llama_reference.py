"""RMSNorm, the gated-SiLU ("SwiGLU") gate and whole transformer blocks with either norm and either feed-forward, restated in
float64 NumPy: the reference of tests/test_gpu_rmsnorm.py, tests/test_gpu_swiglu.py, tests/test_gpu_llama_block.py and of the host
simulator (tests/hostsim/training.py).  The width tables are tests/rowops_reference.py's (``RR``)."""

import numpy as np
import rowops_reference as RR  # noqa: F401  (the tests read the width grid through this module)
from oracle import np_oracle as O

RMS_EPS, LAYER_EPS = 1e-6, 1e-3


def _f64(*arrays):
    return [np.asarray(a, dtype=np.float64) for a in arrays]


# ---- RMSNorm ----------------------------------------------------------------------------------------------------------------
def rmsnorm_fwd(x, gamma, eps=RMS_EPS):
    """(z, rstd [rows, 1]) in float64 on the inputs as given; x is [rows, d] (or [..., d])."""
    x, gamma = _f64(x, gamma)
    rstd = 1.0 / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps)
    return gamma * (x * rstd), rstd


def rmsnorm_bwd(dz, x, gamma, eps=RMS_EPS, residual=None):
    """(dx, dgamma): dx = rstd (g - xh mean(g xh)) [+ residual], g = dz gamma, xh = x rstd; dgamma = sum over rows of dz xh."""
    dz, x, gamma = _f64(dz, x, gamma)
    rstd = 1.0 / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps)
    xh = x * rstd
    g = dz * gamma
    dx = rstd * (g - xh * (g * xh).mean(axis=-1, keepdims=True))
    if residual is not None:
        dx = dx + np.asarray(residual, dtype=np.float64)
    return dx, (dz * xh).reshape(-1, x.shape[-1]).sum(axis=0)


def rmsnorm_ref(x, gamma, dz, residual=None, eps=RMS_EPS):
    """dict z, rstd [rows], dx, dgamma."""
    z, rstd = rmsnorm_fwd(x, gamma, eps)
    dx, dgamma = rmsnorm_bwd(dz, x, gamma, eps, residual)
    return dict(z=z, rstd=rstd[..., 0], dx=dx, dgamma=dgamma)


# ---- the gate ---------------------------------------------------------------------------------------------------------------
def sigmoid(g):
    """float64, overflow-free."""
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        t = np.exp(-np.abs(g))
        return np.where(g >= 0, 1.0 / (1.0 + t), t / (1.0 + t))


def swiglu_fwd(pre):
    """pre [..., 2 U] = gate | up -> h [..., U] = gate sigma(gate) up."""
    pre = np.asarray(pre, dtype=np.float64)
    units = pre.shape[-1] // 2
    g, u = pre[..., :units], pre[..., units:]
    with np.errstate(invalid='ignore', over='ignore'):
        return g * sigmoid(g) * u


def swiglu_bwd(pre, dh):
    """dpre [..., 2 U] = dgate | dup."""
    pre, dh = _f64(pre, dh)
    units = pre.shape[-1] // 2
    g, u = pre[..., :units], pre[..., units:]
    s = sigmoid(g)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.concatenate([dh * u * s * (1.0 + g * (1.0 - s)), dh * (g * s)], axis=-1)


def swiglu_bwd_terms(pre, dh):
    """(T1, T2) = (|dh u sigma|, |dh u g sigma (1 - sigma)|): the magnitudes the bound of dgate is relative to.  1 - sigma is
    sigma(-g), not a subtraction."""
    pre, dh = _f64(pre, dh)
    units = pre.shape[-1] // 2
    g, u = pre[..., :units], pre[..., units:]
    with np.errstate(invalid='ignore', over='ignore'):
        t1 = np.abs(dh * u * sigmoid(g))
        return t1, t1 * np.abs(g) * sigmoid(-g)


# ---- whole blocks -----------------------------------------------------------------------------------------------------------
ATT = ('wq', 'wk', 'wv', 'wo', 'bq', 'bk', 'bv', 'bo')


def parameters(layer):
    """{name: (owner, attribute)} of a TransformerEncoder / TransformerDecoder with any norm and feed-forward."""
    out = {}
    for tag, att in (('sa', layer._self_attention), ('ca', getattr(layer, '_cross_attention', None))):
        if att is not None:
            out.update({f'{tag}.{n}': (att, '_' + n) for n in ATT})
    for i in (1, 2, 3):
        norm = getattr(layer, f'_norm{i}', None)
        if norm is not None:
            out[f'n{i}.gamma'] = (norm, '_gamma')
            if hasattr(norm, '_beta'):
                out[f'n{i}.beta'] = (norm, '_beta')
    lin1 = layer._dense1._linear
    out.update({'w1': (lin1, '_w'), 'b1': (lin1, '_b'), 'w2': (layer._dense2, '_w'), 'b2': (layer._dense2, '_b')})
    return out


def values(layer):
    return {name: np.asarray(getattr(owner, attribute)).astype(np.float64) for name, (owner, attribute) in parameters(layer).items()}


def _norm(p, tag, x, norm, eps):
    """(z, back) with back(dz) -> (dx, grads)."""
    gamma = p[tag + '.gamma']
    if norm == 'rms':
        eps = RMS_EPS if eps is None else eps
        z, _ = rmsnorm_fwd(x, gamma, eps)

        def back(dz):
            dx, dgamma = rmsnorm_bwd(dz, x, gamma, eps)
            return dx, {tag + '.gamma': dgamma}
        return z, back
    eps = LAYER_EPS if eps is None else eps
    beta = p[tag + '.beta']
    mean = x.mean(axis=-1, keepdims=True)
    rstd = 1.0 / np.sqrt(x.var(axis=-1, keepdims=True) + eps)
    yh = (x - mean) * rstd

    def back(dz):
        g = dz * gamma
        dx = rstd * (g - g.mean(axis=-1, keepdims=True) - yh * (g * yh).mean(axis=-1, keepdims=True))
        d = x.shape[-1]
        return dx, {tag + '.gamma': (dz * yh).reshape(-1, d).sum(axis=0), tag + '.beta': dz.reshape(-1, d).sum(axis=0)}
    return gamma * yh + beta, back


def _feed_forward(p, x, ffn):
    shape = x.shape
    x2 = x.reshape(-1, shape[-1])
    pre = x2 @ p['w1'] + p['b1']
    h = swiglu_fwd(pre) if ffn == 'swiglu' else np.maximum(pre, 0.0)
    y = h @ p['w2'] + p['b2']

    def back(dy):
        dy2 = dy.reshape(-1, dy.shape[-1])
        dh = dy2 @ p['w2'].T
        dpre = swiglu_bwd(pre, dh) if ffn == 'swiglu' else np.where(pre >= 0, dh, 0.0)
        grads = {'w2': h.T @ dy2, 'b2': dy2.sum(axis=0), 'w1': x2.T @ dpre, 'b1': dpre.sum(axis=0)}
        return (dpre @ p['w1'].T).reshape(shape), grads
    return y.reshape(shape[:-1] + (y.shape[-1],)), back


def _attention(p, tag, x, memory, mask):
    ap = {n: p[f'{tag}.{n}'] for n in ATT}
    out, cache = O.mha_fwd(ap, x, memory, memory, mask=mask)

    def back(dy):
        (dq, dk, dv), g = O.mha_bwd(ap, cache, dy)
        grads = {f'{tag}.{n}': g[n] for n in ATT}
        if memory is None:
            return dq + dk + dv, None, grads
        return dq, dk + dv, grads
    return out, back


def block_forward(p, x, kv=None, *, norm_first, norm='rms', ffn='swiglu', eps=None, causal=False, masks=None, keep=1.0):
    """A TransformerEncoder (``kv`` None) or TransformerDecoder in float64.  ``masks``: the 0/1 dropout masks of the blocks in
    order (None: no dropout), applied directly in front of each norm.  Returns (out, backward) with
    backward(dy) -> (dx, dkv or None, {name: gradient})."""
    x = np.asarray(x, dtype=np.float64)
    kv = None if kv is None else np.asarray(kv, dtype=np.float64)
    sq = x.shape[1]
    mask = np.tril(np.ones([sq, sq], dtype=bool)) if causal else None
    bodies = [('sa', 'n1')] + ([('ca', 'n2'), ('ff', 'n3')] if kv is not None else [('ff', 'n2')])
    backs = []

    def drop(v, i):
        return v if masks is None else v * np.asarray(masks[i], dtype=np.float64).reshape(v.shape) / keep

    def body(tag, h):
        if tag == 'ff':
            y, back = _feed_forward(p, h, ffn)
            return y, lambda dy: (back(dy)[0], None, back(dy)[1])
        return _attention(p, tag, h, kv if tag == 'ca' else None, mask if tag == 'sa' else None)

    for i, (tag, ntag) in enumerate(bodies):
        if norm_first:
            z, nback = _norm(p, ntag, drop(x, i), norm, eps)
            y, bback = body(tag, z)
            x = x + y
        else:
            y, bback = body(tag, x)
            x, nback = _norm(p, ntag, drop(x + y, i), norm, eps)
        backs.append((i, bback, nback))

    def backward(dy):
        dy = np.asarray(dy, dtype=np.float64)
        grads, dkv = {}, None
        for i, bback, nback in reversed(backs):
            if norm_first:
                dz, dmem, g = bback(dy)
                dn, gn = nback(dz)
                dy = dy + drop(dn, i)
            else:
                dn, gn = nback(dy)
                dn = drop(dn, i)
                db, dmem, g = bback(dn)
                dy = dn + db
            grads.update(g)
            grads.update(gn)
            dkv = dmem if dmem is not None else dkv
        return dy, dkv, grads

    return x, backward
