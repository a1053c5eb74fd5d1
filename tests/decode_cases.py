"""Builders shared by tests/test_decode_host.py (host simulator) and tests/test_gpu_decode.py (MI355X): attention layers and
decoders with O(1) activations, their parameters as float64 dicts for tests/decode_reference.py, and chunked runs."""

import numpy as np

ATT = ('wq', 'wk', 'wv', 'wo', 'bq', 'bk', 'bv', 'bo')
DEC = dict(n1_gamma=('_norm1', '_gamma'), n1_beta=('_norm1', '_beta'), n2_gamma=('_norm2', '_gamma'),
           n2_beta=('_norm2', '_beta'), n3_gamma=('_norm3', '_gamma'), n3_beta=('_norm3', '_beta'),
           d1_w=('_dense1._linear', '_w'), d1_b=('_dense1._linear', '_b'), d2_w=('_dense2', '_w'), d2_b=('_dense2', '_b'))
for _n in ATT:
    DEC['sa_' + _n] = ('_self_attention', '_' + _n)
    DEC['ca_' + _n] = ('_cross_attention', '_' + _n)


def sub(layer, path):
    for part in path.split('.'):
        layer = getattr(layer, part)
    return layer


def chunkings(seq):
    """The whole sequence at once, token by token, and ragged chunks 5, 1, 1, 3, 5, 1, 1, 3, ..."""
    ragged, left, i = [], seq, 0
    while left:
        ragged.append(min((5, 1, 1, 3)[i % 4], left))
        left -= ragged[-1]
        i += 1
    return [[seq], [1] * seq, ragged]


def split(x, sizes):
    edges = np.cumsum([0] + list(sizes))
    return [x[:, a:b] for a, b in zip(edges[:-1], edges[1:])]


def make_mha(npm, features, heads, kv_heads, seed, batch=2):
    """An initialised MultiHeadAttention with weights scaled to O(1) scores; (layer, float64 parameter dict)."""
    np.random.seed(seed)
    att = npm.layers.MultiHeadAttention(heads, num_kv_heads=kv_heads)
    att(np.zeros([batch, 2, features], dtype=np.float32))
    for name in ('_wq', '_wk', '_wv', '_wo'):
        arr = getattr(att, name)
        arr.set(np.asarray(arr) * np.float32(2.0 / np.sqrt(features)))
    return att, {n: np.asarray(getattr(att, '_' + n)).astype(np.float64) for n in ATT}


def run_mha_chunks(att, x, sizes, capacity):
    """``x`` fed through ``att`` in chunks with a fresh cache; the outputs concatenated, and the path each chunk took."""
    cache = att.make_cache(x.shape[0], capacity)
    outs, paths = [], []
    for piece in split(x, sizes):
        outs.append(np.asarray(att(np.ascontiguousarray(piece), cache=cache)))
        paths.append(att._cached_path)
    assert cache.length == sum(sizes)
    return np.concatenate(outs, axis=1), paths


def make_decoder(npm, features, heads, kv_heads, hidden, norm_first, causal, seed, batch=2, seq_kv=7):
    np.random.seed(seed)
    dec = npm.layers.TransformerDecoder(num_heads=heads, hidden_units=hidden, norm_first=norm_first, num_kv_heads=kv_heads,
                                        causal=causal)
    dec(np.zeros([batch, 2, features], dtype=np.float32), np.zeros([batch, seq_kv, features], dtype=np.float32))
    for path, attrs in (('_self_attention', ('_wq', '_wk', '_wv', '_wo')), ('_cross_attention', ('_wq', '_wk', '_wv', '_wo')),
                        ('_dense1._linear', ('_w',)), ('_dense2', ('_w',))):
        for attr in attrs:
            arr = getattr(sub(dec, path), attr)
            arr.set(np.asarray(arr) * np.float32(2.0 / np.sqrt(features)))
    return dec, decoder_params(dec)


def decoder_params(dec):
    return {k: np.asarray(getattr(sub(dec, path), attr)).astype(np.float64) for k, (path, attr) in DEC.items()}


def run_decoder_chunks(dec, q, kv, sizes, capacity):
    state = dec.start_decoding(kv, capacity)
    outs = [np.asarray(dec.decode(np.ascontiguousarray(piece), state)) for piece in split(q, sizes)]
    assert state.position == sum(sizes) and state.cross_cache.length == kv.shape[1]
    return np.concatenate(outs, axis=1)


class GradRecorder:
    """An optimizer that records gradients instead of applying them (parameters stay fixed)."""

    def __init__(self):
        self.grads = {}

    def update(self, obj, attribute, gradient):
        self.grads[(id(obj), attribute)] = np.array(gradient, dtype=np.float64, copy=True)

    def named(self, dec):
        return {k: self.grads[(id(sub(dec, path)), attr)] for k, (path, attr) in DEC.items()}
