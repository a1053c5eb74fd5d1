"""GPU: npm_take_rows and npm_embedding_bwd (csrc/npm_rowops.hip) and ``layers.Embedding`` on them.

Bounds.  npm_take_rows is a copy: rows are compared as uint32 with NumPy indexing.  npm_embedding_bwd sums the ``dy`` rows of a
token in ascending row order in fp32: bit for bit a NumPy float32 loop in that order, and within 1e-6 (1 + max |ref|) of
``np.add.at`` in float64 (at most 196 additions of O(1) terms per token here: 196 * 2^-24 * |partial sums| stays below it).  The
optimizer steps: SGD is one fp32 axpy on that gradient (1e-6 against NumPy); Adam at its first step moves every parameter with a
nonzero gradient by lr * sign(g) up to the epsilon inside the root (1e-5).

Every test here needs ``npm_take_rows``, ``npm_embedding_bwd`` or ``layers.Embedding``: none passes on the parent commit.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('cols', [1, 3, 4, 64, 1027])
def test_take_rows_is_numpy_indexing_with_zero_rows_outside(npm, cols):
    from np_modeling_amd import _C, device as D
    rng = np.random.default_rng(cols)
    src_rows, guard = 37, 3
    table = rng.standard_normal([src_rows, cols]).astype(np.float32)
    idx = np.concatenate([[-1, src_rows, 0, src_rows - 1, 5, 5, 5, -7, src_rows + 100], rng.integers(0, src_rows, size=300)])
    inside = (idx >= 0) & (idx < src_rows)
    want = np.where(inside[:, None], table[np.clip(idx, 0, src_rows - 1)], np.float32(0))
    got = D.take_rows(D.from_host(table), idx).numpy()
    assert got.shape == (idx.size, cols) and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(D.take_rows(D.from_host(table), D.ids_from_host(idx.reshape(3, 103))).numpy()), bits(want.reshape(3, 103, cols)))
    # a pitched destination: the guard columns keep their sentinel; a pitched source: its padding is never copied
    index = D.ids_from_host(idx)
    for pad in (guard, 4):
        pitch = cols + pad
        dst = D.from_host(np.full([idx.size, pitch], np.float32(-7.5)))
        src = D.from_host(np.concatenate([table, np.full([src_rows, pad], np.float32(np.nan))], axis=1))
        _C.check(_C.lib().npm_take_rows(src.ptr, pitch, src_rows, index.ptr, dst.ptr, pitch, idx.size, cols), 'npm_take_rows')
        out = dst.numpy()
        assert np.array_equal(bits(out[:, :cols]), bits(want)) and (out[:, cols:] == np.float32(-7.5)).all()


def _fp32_loop(ids, dy, vocab):
    want = np.zeros([vocab, dy.shape[1]], dtype=np.float32)
    seen = set()
    for r, token in enumerate(ids):
        want[token] = dy[r] if token not in seen else want[token] + dy[r]
        seen.add(token)
    return want


@pytest.mark.parametrize('case', ['six', 'two-hundred'])
@pytest.mark.parametrize('features', [6, 300])
def test_embedding_backward_is_the_fp32_loop_in_row_order(npm, case, features):
    from decode_cases import GradRecorder
    rng = np.random.default_rng(features)
    vocab = 12
    ids = np.array([3, 3, 3, 0, 7, 3]) if case == 'six' else rng.choice([1, 4, 5, 9, 11], size=200, p=[0.9, 0.04, 0.03, 0.02, 0.01])
    if case == 'two-hundred':
        ids[[0, 50, 100, 150, 199]] = [11, 9, 5, 4, 1]                              # all five occur, whatever was drawn
        assert len(set(ids.tolist())) == 5
    np.random.seed(1)
    emb = npm.layers.Embedding(vocab, features)
    y = emb(ids)
    table = emb.w.numpy()
    assert np.array_equal(bits(y.numpy()), bits(table[ids]))
    dy = rng.standard_normal([ids.size, features]).astype(np.float32)
    recorder = GradRecorder()
    emb(dy, backprop=True, optimizer_=recorder)
    got = recorder.grads[(id(emb), '_w')].astype(np.float32)
    assert np.array_equal(bits(got), bits(_fp32_loop(ids.tolist(), dy, vocab)))
    want = np.zeros([vocab, features])
    np.add.at(want, ids, dy.astype(np.float64))
    assert np.abs(got - want).max() <= 1e-6 * (1 + np.abs(want).max())
    assert np.array_equal(emb.w.numpy(), table)                                  # the recorder applied nothing


def test_one_sgd_step_and_one_adam_step(npm):
    rng = np.random.default_rng(5)
    ids = np.array([[3, 3, 9], [0, 7, 3]])
    dy = rng.standard_normal([2, 3, 8]).astype(np.float32)
    grad = np.zeros([10, 8])
    np.add.at(grad, ids.reshape(-1), dy.reshape(-1, 8).astype(np.float64))
    for name in ('sgd', 'adam'):
        np.random.seed(2)
        emb = npm.layers.Embedding(10, 8)
        emb(ids)
        table = emb.w.numpy().astype(np.float64)
        if name == 'sgd':
            emb(dy, backprop=True, learning_rate=0.1)
            want = table - 0.1 * grad
            tol = 1e-6
        else:
            emb(dy, backprop=True, optimizer_=npm.optimizer.AdamOptimizer(0.01))
            m, v = 0.1 * grad, 0.001 * grad * grad                               # the first step from zero moments
            want = table - 0.01 * (m / 0.1) / np.sqrt(v / 0.001 + 1e-7)
            tol = 1e-5
        assert np.abs(emb.w.numpy() - want).max() <= tol * (1 + np.abs(want).max()), name
