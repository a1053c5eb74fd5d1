"""CPU: the host side of ``loss.SoftmaxCrossEntropyLoss`` and of the two ``Trainer`` hooks, on the host simulator (tests/hostsim/;
npm_softmax_xent_rows joins it with the profile 'xent')."""

import contextlib
import io

import hostsim
import numpy as np
import pytest
import xent_reference
from hostsim.fixtures import npm_fixture

npm = npm_fixture()


def _logits(rows=6, vocab=11, seed=0, lead=None):
    rng = np.random.default_rng(seed)
    shape = (rows, vocab) if lead is None else tuple(lead) + (vocab,)
    return (3 * rng.standard_normal(shape)).astype(np.float32)


# ---- validation ---------------------------------------------------------------------------------------------------------------

def test_constructor_rejects_what_it_cannot_mean(npm):
    from np_modeling_amd import loss
    for kwargs in ({'label_smoothing': 1.0}, {'label_smoothing': -0.1}, {'reduction': 'none'}, {'ignore_index': 1.5}, {'ignore_index': True}):
        with pytest.raises(ValueError):
            loss.SoftmaxCrossEntropyLoss(**kwargs)


def test_host_targets_are_validated(npm):
    from np_modeling_amd import device as D, loss
    z = D.from_host(_logits())
    xent = loss.SoftmaxCrossEntropyLoss()
    good = np.arange(6) % 11
    with pytest.raises(ValueError, match='integers'):
        xent.forward(z, good.astype(np.float32))
    with pytest.raises(ValueError, match='integers'):
        xent.forward(z, good > 2)
    with pytest.raises(ValueError, match='do not match'):
        xent.forward(z, good[:5])
    with pytest.raises(ValueError, match='do not match'):
        xent.forward(z, good.reshape(2, 3))
    with pytest.raises(ValueError, match='outside the vocabulary'):
        xent.forward(z, np.where(good == 3, 11, good))
    with pytest.raises(ValueError, match='not ignore_index'):
        xent.forward(z, np.where(good == 3, -2, good))
    with pytest.raises(ValueError, match='not ignore_index'):
        loss.SoftmaxCrossEntropyLoss(ignore_index=-100).forward(z, np.where(good == 3, -1, good))
    with pytest.raises(ValueError, match='not ignore_index'):
        loss.SoftmaxCrossEntropyLoss(ignore_index=0).forward(z, np.where(good == 3, -1, good))
    assert npm.sim.calls.count('npm_softmax_xent_rows') == 0            # nothing was launched on the way
    with pytest.raises(ValueError, match=r'\[\.\.\., V\]'):
        xent.forward(D.empty([]), good)


def test_an_id_buffer_takes_only_a_negative_ignore_index_and_its_own_shape(npm):
    from np_modeling_amd import device as D, loss
    z = D.from_host(_logits())
    ids = D.ids_from_host(np.arange(6) % 11)
    with pytest.raises(ValueError, match='IdBuffer'):
        loss.SoftmaxCrossEntropyLoss(ignore_index=0).forward(z, ids)
    with pytest.raises(ValueError, match='do not match'):
        loss.SoftmaxCrossEntropyLoss().forward(z, D.ids_from_host(np.arange(5)))
    assert np.isfinite(loss.SoftmaxCrossEntropyLoss(ignore_index=-100).forward(z, ids))


def test_backward_needs_a_gradient_and_perplexity_no_smoothing(npm):
    from np_modeling_amd import device as D, loss
    z, t = D.from_host(_logits()), np.arange(6) % 11
    xent = loss.SoftmaxCrossEntropyLoss()
    with pytest.raises(RuntimeError, match='need_grad'):
        xent.backward()
    xent.forward(z, t)
    assert xent.backward().shape == z.shape
    xent.forward(z, t, need_grad=False)
    with pytest.raises(RuntimeError, match='need_grad'):
        xent.backward()
    smooth = loss.SoftmaxCrossEntropyLoss(label_smoothing=0.1)
    smooth.forward(z, t)
    with pytest.raises(RuntimeError, match='label_smoothing'):
        smooth.perplexity()


def test_a_library_without_the_entry_point_is_an_error_that_names_it():
    from np_modeling_amd import _C, device as D, loss
    hostsim.install('logits')                       # the library from just before the feature: the symbol is missing
    try:
        with pytest.raises(_C.NpmError, match='npm_softmax_xent_rows'):
            loss.SoftmaxCrossEntropyLoss().forward(D.from_host(_logits()), np.arange(6))
    finally:
        hostsim.uninstall()


# ---- values -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('reduction', ['mean', 'sum'])
@pytest.mark.parametrize('smoothing', [0.0, 0.2])
def test_reductions_count_and_the_per_row_results(npm, reduction, smoothing):
    from np_modeling_amd import device as D, loss
    host = _logits(lead=(2, 4), vocab=9, seed=1)
    t = np.array([[0, 8, -1, 3], [-1, -1, 5, 2]])
    xent = loss.SoftmaxCrossEntropyLoss(label_smoothing=smoothing, reduction=reduction)
    value = xent.forward(D.from_host(host), t)
    scale = 1.0 / 5 if reduction == 'mean' else 1.0
    ref = xent_reference.reference(host.reshape(8, 9), t.reshape(8), smoothing, scale)
    assert xent.count == 5 and isinstance(value, np.float64)
    row_loss32 = ref.row_loss.astype(np.float32)
    assert value == pytest.approx(row_loss32.astype(np.float64).sum() * scale, rel=1e-12)
    assert xent.row_loss.shape == (2, 4) and xent.lse.shape == (2, 4)
    np.testing.assert_array_equal(xent.row_loss.numpy().reshape(8), row_loss32)
    np.testing.assert_array_equal(xent.lse.numpy().reshape(8), ref.lse.astype(np.float32))
    grad = xent.backward()
    assert grad.shape == (2, 4, 9)
    np.testing.assert_array_equal(grad.numpy().reshape(8, 9), ref.grad.astype(np.float32))
    assert not grad.numpy()[0, 2].any() and not grad.numpy()[1, 0].any()           # ignored rows: zeros
    if smoothing == 0.0:
        assert xent.perplexity() == pytest.approx(np.exp(row_loss32.astype(np.float64).sum() / 5), rel=1e-12)


def test_no_valid_target_divides_by_one(npm):
    from np_modeling_amd import device as D, loss
    xent = loss.SoftmaxCrossEntropyLoss()
    value = xent.forward(D.from_host(_logits()), np.full(6, -1))
    assert value == 0.0 and xent.count == 0 and xent.perplexity() == 1.0
    assert not xent.backward().numpy().any() and not xent.row_loss.numpy().any()


def test_zero_rows(npm):
    from np_modeling_amd import device as D, loss
    xent = loss.SoftmaxCrossEntropyLoss()
    assert xent.forward(D.empty([0, 7]), np.zeros([0], dtype=np.int64)) == 0.0
    assert xent.count == 0 and xent.backward().shape == (0, 7)
    assert npm.sim.npm_last_xent_kernel() == b'xent_none rows=0'


def test_a_non_negative_ignore_index_becomes_minus_one_on_the_host(npm):
    from np_modeling_amd import device as D, loss
    host, t = _logits(), np.array([0, 3, 10, 3, 7, 12])        # 12: beyond the vocabulary, legal because it is the pad id
    a = loss.SoftmaxCrossEntropyLoss(ignore_index=12)
    b = loss.SoftmaxCrossEntropyLoss()
    va, vb = a.forward(D.from_host(host), t), b.forward(D.from_host(host), np.where(t == 12, -1, t))
    assert va == vb and a.count == b.count == 5
    np.testing.assert_array_equal(a.backward().numpy(), b.backward().numpy())
    inside = loss.SoftmaxCrossEntropyLoss(ignore_index=3)      # a pad id inside the vocabulary
    inside.forward(D.from_host(host), t[:5].tolist() + [3])
    assert inside.count == 3 and not inside.backward().numpy()[[1, 3, 5]].any()


def test_host_targets_are_read_every_forward_and_uploaded_when_they_change(npm):
    from np_modeling_amd import device as D, loss
    z, t = D.from_host(_logits()), np.arange(6) % 11
    xent = loss.SoftmaxCrossEntropyLoss()
    before = len(npm.sim.uploads)
    first = xent.forward(z, t)
    assert npm.sim.uploads[before:] == [24]                         # six int32
    assert xent.forward(z, t) == first
    assert npm.sim.uploads[before:] == [24]                         # same object, same contents: no second upload
    t[2] = 9                                                    # refilled in place: noticed, because the array is read again
    assert xent.forward(z, t) != first
    assert npm.sim.uploads[before:] == [24, 24]
    xent.forward(z, t.copy())                                   # another object
    assert npm.sim.uploads[before:] == [24, 24, 24]
    t[2] = 11
    with pytest.raises(ValueError, match='outside the vocabulary'):
        xent.forward(z, t)


def test_an_id_buffer_is_counted_once_per_object(npm):
    from np_modeling_amd import device as D, loss
    z = D.from_host(_logits())
    ids = D.ids_from_host(np.array([1, -1, 4, -5, 0, 2]))
    xent = loss.SoftmaxCrossEntropyLoss()
    before = len(npm.sim.d2h)
    xent.forward(z, ids)
    xent.forward(z, ids)
    assert xent.count == 4 and npm.sim.d2h[before:] == [24]
    xent.forward(z, D.ids_from_host(np.array([1, 1, 4, 5, 0, 2])))
    assert xent.count == 6 and npm.sim.d2h[before:] == [24, 24]


def test_inplace_returns_the_logits_buffer(npm):
    from np_modeling_amd import device as D, loss
    host, t = _logits(), np.arange(6) % 11
    z = D.from_host(host)
    fresh = loss.SoftmaxCrossEntropyLoss()
    value = fresh.forward(z, t)
    assert fresh.backward().ptr != z.ptr
    np.testing.assert_array_equal(z.numpy(), host)              # untouched
    over = loss.SoftmaxCrossEntropyLoss(inplace=True)
    assert over.forward(z, t) == value
    assert over.backward() is z
    np.testing.assert_array_equal(z.numpy(), fresh.backward().numpy())
    assert b'inplace=1' in npm.sim.npm_last_xent_kernel()


def test_evaluation_is_one_call_and_no_rows_by_vocab_buffer(npm):
    from np_modeling_amd import device as D, loss
    rows, vocab = 16, 4096
    z, ids = D.from_host(_logits(rows, vocab)), D.ids_from_host(np.arange(rows))
    xent = loss.SoftmaxCrossEntropyLoss()
    xent.forward(z, ids, need_grad=False)                       # the count of this buffer is known from here on
    calls, live = len(npm.sim.calls), npm.sim.live
    npm.sim.peak = npm.sim.live
    value = xent.forward(z, ids, need_grad=False)
    assert npm.sim.calls[calls:] == ['npm_softmax_xent_rows']
    assert npm.sim.peak - live < 4 * rows * vocab and npm.sim.peak - live <= 2 * (8 * rows + 64)
    assert b'grad=0' in npm.sim.npm_last_xent_kernel()
    with_grad = xent.forward(z, ids)
    assert with_grad == value and npm.sim.peak - live >= 4 * rows * vocab


def test_finite_differences_of_the_restatement():
    rng = np.random.default_rng(5)
    z = 2 * rng.standard_normal((4, 7))
    z[1, 2] = -np.inf
    t = np.array([3, 0, -1, 6])
    for smoothing in (0.0, 0.25):
        rows = [0, 2, 3] if smoothing else [0, 1, 2, 3]          # row 1 has a masked token: its smoothed loss is +inf
        ref = xent_reference.reference(z, t, smoothing, 0.5)
        for r in rows:
            for j in range(7):
                if not np.isfinite(z[r, j]):
                    assert ref.grad[r, j] == 0.0
                    continue
                h = 1e-6
                up, down = z.copy(), z.copy()
                up[r, j] += h
                down[r, j] -= h
                slope = (xent_reference.reference(up, t, smoothing).row_loss[r] - xent_reference.reference(down, t, smoothing).row_loss[r]) / (2 * h)
                assert ref.grad[r, j] == pytest.approx(0.5 * slope, abs=1e-8)


def test_host_logits_take_the_numpy_path_with_the_same_rules(npm):
    from np_modeling_amd import loss
    host = _logits(7, 13, seed=2).astype(np.float64)
    host[1, 4:9] = -np.inf
    host[2, 3] = np.nan
    host[5] = -np.inf
    t = np.array([0, 12, 1, -1, 5, 2, 4])
    calls = len(npm.sim.calls)
    for smoothing in (0.0, 0.1):
        xent = loss.SoftmaxCrossEntropyLoss(label_smoothing=smoothing, reduction='sum')
        value = xent.forward(host, t)
        ref = xent_reference.reference(host, t, smoothing, 1.0)
        np.testing.assert_allclose(xent.row_loss, ref.row_loss, rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(xent.lse, ref.lse, rtol=1e-13)
        np.testing.assert_allclose(xent.backward(), ref.grad, rtol=1e-12, atol=1e-15)
        assert np.isnan(value) and xent.count == 6
    clean = loss.SoftmaxCrossEntropyLoss()
    value = clean.forward(host[[0, 1, 3, 4, 6]], t[[0, 1, 3, 4, 6]])
    ref = xent_reference.reference(host[[0, 1, 3, 4, 6]], t[[0, 1, 3, 4, 6]], 0.0, 1 / 4)
    assert value == pytest.approx(ref.loss_sum / 4, rel=1e-13) and clean.perplexity() == pytest.approx(np.exp(ref.loss_sum / 4), rel=1e-13)
    np.testing.assert_allclose(clean.backward(), ref.grad, rtol=1e-12, atol=1e-15)
    assert npm.sim.calls[calls:] == []                              # nothing ran on the device


# ---- Trainer ------------------------------------------------------------------------------------------------------------------

_STEP = ['npm_sgemm'] * 4 + ['npm_axpy'] + ['npm_sgemm'] * 2 + ['npm_axpy']
# what three steps of the two models below record at the commit before the hooks existed: (calls, uploads, d2h)
_PARENT_TRACE = {
    'mse': (_STEP * 3, [120, 72, 140, 28, 84, 12], []),
    'xent': (_STEP * 3, [120, 96, 140, 28, 112, 16], []),
}


@pytest.mark.parametrize('which', ['mse', 'xent'])
def test_trainer_without_the_hooks_records_what_it_always_did(npm, which):
    from np_modeling_amd import layers, loss, optimizer, train
    np.random.seed(3)
    x = np.random.normal(size=(6, 5)).astype(np.float32)
    if which == 'mse':
        model = [layers.mlp.Dense(7), layers.mlp.Linear(3)]
        y = np.random.normal(size=(6, 3)).astype(np.float32)
        loss_ = loss.MSELoss()
    else:
        model = [layers.mlp.Dense(7), layers.mlp.Linear(4), layers.activations.Softmax()]
        y = np.eye(4, dtype=np.float32)[np.arange(6) % 4]
        loss_ = loss.CrossEntropyLoss()
    assert not hasattr(loss_, 'resident_targets') and not hasattr(model[0], 'resident_inputs')
    with contextlib.redirect_stdout(io.StringIO()):
        train.Trainer(model, loss_).train(x, y, 3, optimizer.SGDOptimizer(0.1))
    assert (list(npm.sim.calls), list(npm.sim.uploads), list(npm.sim.d2h)) == _PARENT_TRACE[which]


def test_trainer_keeps_token_ids_integers_and_uploads_them_once(npm):
    from np_modeling_amd import device as D, layers, loss, optimizer, train
    np.random.seed(4)
    vocab, batch, seq = 12, 3, 5
    tokens = np.random.randint(0, vocab, size=(batch, seq + 1))
    tokens[1, 4:] = -1                                          # a shorter sequence, padded
    # Linear's backward is 2-D, as the reference's: one row per token
    inputs, targets = tokens[:, :-1].reshape(-1), tokens[:, 1:].reshape(-1)
    embedding = layers.embedding.Embedding(vocab, 8)
    seen = []
    forward = embedding.forward
    embedding.forward = lambda ids: (seen.append(ids), forward(ids))[1]
    xent = loss.SoftmaxCrossEntropyLoss()
    trainer = train.Trainer([embedding, layers.mlp.Dense(16), layers.mlp.Linear(vocab)], xent)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        trainer.train(inputs, targets, 3, optimizer.SGDOptimizer(0.5))
    assert len(seen) == 3 and all(isinstance(ids, D.IdBuffer) for ids in seen) and seen[0] is seen[1] is seen[2]
    np.testing.assert_array_equal(seen[0].numpy(), inputs)
    assert npm.sim.uploads.count(4 * batch * seq) == 2              # the inputs once, the targets once: never again in three steps
    assert npm.sim.calls.count('npm_softmax_xent_rows') == 3
    assert xent.count == int((targets >= 0).sum())
    values = [float(line.split()[-1]) for line in out.getvalue().splitlines() if line.startswith('Loss:')]
    assert len(values) == 3 and values[2] < values[1] < values[0]
    # the checks of host targets run in resident_targets and, for the id range, at the first forward
    with pytest.raises(ValueError, match='integers'):
        trainer.train(inputs, targets.astype(np.float32), 1, optimizer.SGDOptimizer(0.5))
    with pytest.raises(ValueError, match='outside the vocabulary'):
        with contextlib.redirect_stdout(io.StringIO()):
            trainer.train(inputs, np.where(np.arange(targets.size) == 2, vocab, targets), 1, optimizer.SGDOptimizer(0.5))
    # eval: no gradient
    calls = len(npm.sim.calls)
    with contextlib.redirect_stdout(io.StringIO()):
        trainer.eval(inputs, targets)
    assert b'grad=0' in npm.sim.npm_last_xent_kernel() and npm.sim.calls[calls:].count('npm_softmax_xent_rows') == 1
    with pytest.raises(RuntimeError):
        xent.backward()


@pytest.mark.parametrize('pad', [0, 5, 12, 40])
def test_trainer_with_a_non_negative_pad_id_is_the_minus_one_run(npm, pad):
    """``resident_targets`` maps the pad id to -1 once; the forward must take that buffer although ``ignore_index >= 0``.  Pad ids
    inside (0, 5) and beyond (12, 40) the vocabulary of 12; count, every loss and the last gradient equal the run with -1."""
    from np_modeling_amd import layers, loss, optimizer, train
    vocab = 12
    rng = np.random.default_rng(9)
    inputs = rng.integers(0, vocab, size=15)
    real = rng.integers(0, vocab, size=15)
    real[real == pad] = (pad + 1) % vocab                       # no real target equals the pad id
    padded = np.arange(15) % 4 == 3

    def run(loss_, targets):
        np.random.seed(8)
        model = [layers.embedding.Embedding(vocab, 8), layers.mlp.Dense(16), layers.mlp.Linear(vocab)]
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            train.Trainer(model, loss_).train(inputs, targets, 3, optimizer.SGDOptimizer(0.5))
        values = [float(line.split()[-1]) for line in out.getvalue().splitlines() if line.startswith('Loss:')]
        return values, loss_.count, loss_.backward().numpy()

    uploads = len(npm.sim.uploads)
    values, count, grad = run(loss.SoftmaxCrossEntropyLoss(ignore_index=pad), np.where(padded, pad, real))
    assert npm.sim.uploads[uploads:].count(60) == 2                 # inputs and targets once each, mapped on the host
    want_values, want_count, want_grad = run(loss.SoftmaxCrossEntropyLoss(), np.where(padded, -1, real))
    assert count == want_count == int((~padded).sum()) and len(values) == 3 and values == want_values
    np.testing.assert_array_equal(grad, want_grad)
    assert not grad[padded].any() and grad[~padded].any()
    # a caller's own IdBuffer is still refused with a non-negative ignore_index, also right after a Trainer run
    from np_modeling_amd import device as D
    xent = loss.SoftmaxCrossEntropyLoss(ignore_index=pad)
    xent.resident_targets(np.where(padded, pad, real))
    with pytest.raises(ValueError, match='IdBuffer'):
        xent.forward(D.from_host(_logits(15, vocab)), D.ids_from_host(real))


def test_trainer_eval_leaves_a_loss_without_need_grad_alone(npm):
    from np_modeling_amd import layers, loss, train
    np.random.seed(5)
    x, y = np.random.normal(size=(4, 5)).astype(np.float32), np.random.normal(size=(4, 3)).astype(np.float32)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        train.Trainer([layers.mlp.Linear(3)], loss.MSELoss()).eval(x, y)
    assert out.getvalue().startswith('Loss: ')
