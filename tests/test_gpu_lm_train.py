"""GPU: a small language model trained from token ids by ``Trainer`` with ``loss.SoftmaxCrossEntropyLoss`` -- ``Embedding(50, 32)`` ->
``TransformerDecoder`` (2 heads, hidden 64, norm_first, causal) over a fixed memory -> ``Linear(50)`` -- on ragged sequences
padded with -1.

Bounds.  The first step is compared with the same model run through what a user had to write before: ``Softmax`` +
``CrossEntropyLoss`` over one-hot float targets (zero rows where padded), the loss sum and its gradient divided by the count.  Both
run the same fp32 kernels below the logits, so the loss and every parameter gradient are held to the project's parity contract
(include/npm_hip.h NPM_PARITY_REL_F32 on the elements of at least 0.1 of the tensor's maximum, NPM_PARITY_SCALED_F32 on all) with
the composition as the reference.  Generation is greedy: before tokens are compared the test asserts that every top-2 logit gap of
the teacher-forced run is at least GAP of max |logit|, the margin tests/test_gpu_spec.py asks of its fixture.

Every test here needs ``SoftmaxCrossEntropyLoss`` and the ``Trainer`` hooks: none passes on the parent commit."""

import contextlib
import copy
import io

import numpy as np
import pytest

import decode_cases as DC

pytestmark = pytest.mark.gpu

B, S, F, HEADS, HIDDEN, VOCAB, SEQ_KV = 3, 6, 32, 2, 64, 50, 7
LENGTHS = (7, 4, 6)                    # tokens per sequence: S + 1 at most (inputs are all but the last, targets all but the first)
STEPS, LR = 8, 0.045                   # plain SGD: at 0.04 .. 0.05 every step lowers the loss by 0.1 or more, from 0.06 on one does not
GAP = 1e-3


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


def _layers(npm, dec, kv):
    """The two adapters a sequential ``Trainer`` needs around the decoder and the 2-D ``Linear``."""
    from np_modeling_amd.layers.layer import Layer

    class OverMemory(Layer):
        def forward(self, x):
            return dec(x, kv)

        def backward(self, dy, optimizer_):
            return dec(dy, backprop=True, optimizer_=optimizer_)[0]

    class Rows(Layer):
        def forward(self, x):
            self._shape = x.shape
            return x.reshape(-1, x.shape[-1])

        def backward(self, dy, optimizer_):
            return dy.reshape(self._shape)

    return OverMemory(), Rows()


def build(npm):
    dec, _ = DC.make_decoder(npm, F, HEADS, HEADS, HIDDEN, norm_first=True, causal=True, seed=60, batch=B, seq_kv=SEQ_KV)
    np.random.seed(61)
    emb = npm.layers.Embedding(VOCAB, F)
    emb(np.zeros([1], dtype=np.int64))
    head = npm.layers.Linear(units=VOCAB)
    head(np.zeros([1, F], dtype=np.float32))
    head._w.set(np.asarray(head._w) * np.float32(0.5 / np.sqrt(F)))         # a first loss near log(VOCAB)
    rng = np.random.default_rng(62)
    kv = rng.standard_normal([B, SEQ_KV, F]).astype(np.float32)
    tokens = np.full([B, S + 1], -1, dtype=np.int64)
    for b, n in enumerate(LENGTHS):
        tokens[b, :n] = rng.permutation(VOCAB)[:n]              # no token twice in a sequence
    return {'emb': emb, 'dec': dec, 'head': head, 'kv': kv, 'tokens': tokens,
            'inputs': tokens[:, :-1].copy(), 'targets': tokens[:, 1:].reshape(-1).copy()}


class Recorder:
    """An optimizer that keeps every gradient, in the order the backward hands them over, and changes nothing."""

    def __init__(self):
        self.grads = []

    def update(self, obj, attribute, gradient):
        self.grads.append((type(obj).__name__ + '.' + attribute, np.array(gradient, dtype=np.float64, copy=True)))


def _trainer(npm, model, loss_):
    over, rows = _layers(npm, model['dec'], model['kv'])
    return npm.train.Trainer([model['emb'], over, rows, model['head']], loss_)


def _losses(text):
    return [float(line.split()[-1]) for line in text.splitlines() if line.startswith('Loss:')]


def _parity(got, ref, what):
    from np_modeling_amd import _C
    rel_bound, scaled_bound = _C.parity_bounds()['f32']
    top = np.abs(ref).max()
    err = np.abs(got - ref)
    big = np.abs(ref) >= 0.1 * top
    scaled, rel = float(err.max() / top), float((err[big] / np.abs(ref[big])).max())
    print(f'{what}: rel {rel:.2e} scaled {scaled:.2e}')
    assert scaled <= scaled_bound and rel <= rel_bound, (what, rel, scaled)


def test_the_first_step_is_the_one_hot_composition(npm):
    from np_modeling_amd import device as D
    model = build(npm)
    old = copy.deepcopy({k: model[k] for k in ('emb', 'dec', 'head')})
    count = int((model['targets'] >= 0).sum())
    assert count == sum(LENGTHS) - B

    # what a user had to write
    softmax, xent, theirs = npm.layers.Softmax(), npm.loss.CrossEntropyLoss(), Recorder()
    one_hot = np.zeros([B * S, VOCAB], dtype=np.float32)
    live = np.flatnonzero(model['targets'] >= 0)
    one_hot[live, model['targets'][live]] = 1.0
    hidden = old['dec'](old['emb'](model['inputs']), model['kv'])
    their_loss = xent(softmax(old['head'](hidden.reshape(-1, F))), one_hot) / count
    dlogits = softmax(D.as_device(xent(backprop=True) * (1.0 / count)), backprop=True)
    dhidden = old['head'](dlogits, backprop=True, optimizer_=theirs)
    dx = old['dec'](dhidden.reshape(B, S, F), backprop=True, optimizer_=theirs)[0]
    old['emb'](dx, backprop=True, optimizer_=theirs)

    # the same through Trainer and the new loss
    ours, out = Recorder(), io.StringIO()
    new_loss = npm.loss.SoftmaxCrossEntropyLoss()
    with contextlib.redirect_stdout(out):
        _trainer(npm, model, new_loss).train(model['inputs'], model['targets'], 1, ours)
    (our_loss,) = _losses(out.getvalue())
    assert new_loss.count == count
    from np_modeling_amd import _C
    print(f'first-step loss: ours {our_loss:.9g} theirs {their_loss:.9g}')
    assert abs(our_loss - their_loss) <= _C.parity_bounds()['f32'][0] * abs(their_loss)
    assert [name for name, _ in ours.grads] == [name for name, _ in theirs.grads] and len(ours.grads) >= 20
    for (name, got), (_, ref) in zip(ours.grads, theirs.grads):
        if name.endswith('._bk'):       # exactly zero in real arithmetic (the rows of the score gradient sum to 0): rounding noise in
            assert np.abs(got).max() < 1e-4 and np.abs(ref).max() < 1e-4           # both, as tests/test_gpu_encoder.py treats it
            continue
        _parity(got, ref, name)
    rows = new_loss.backward().numpy()
    assert not rows[model['targets'] < 0].any()                 # the padded positions: zero gradient rows


def _teacher_forced_logits(model):
    hidden = model['dec'](model['emb'](model['inputs']), model['kv'])
    return model['head'](hidden.reshape(-1, F)).numpy().reshape(B, S, VOCAB)


def _greedy(npm, model, prompt_len, steps):
    """tests/test_gpu_generate.py's loop: sampler -> Embedding.forward(result.ids) -> decode on a paged cache -> take_rows -> head."""
    from np_modeling_amd import device as D
    dec, emb, head = model['dec'], model['emb'], model['head']
    lengths = np.full(B, prompt_len)
    state = dec.start_decoding(model['kv'], 16, page_size=16, pages=B)
    sampler = npm.sampling.Sampler(B)
    x = emb.forward(model['tokens'][:, :prompt_len])
    new_lengths, last = lengths, np.arange(B) * prompt_len + lengths - 1
    tokens = []
    for _ in range(steps):
        hidden = dec.decode(x, state, new_lengths=new_lengths)
        result = sampler(head(D.take_rows(hidden.reshape(-1, F), last)))
        x = emb.forward(result.ids).reshape(B, 1, F)
        tokens.append(result.numpy().tolist())
        new_lengths, last = None, np.arange(B)
    return np.array(tokens).T                                   # [B, steps]


def test_eight_steps_learn_the_batch_and_greedy_generation_continues_it(npm):
    model = build(npm)
    out = io.StringIO()
    loss_ = npm.loss.SoftmaxCrossEntropyLoss()
    trainer = _trainer(npm, model, loss_)
    with contextlib.redirect_stdout(out):
        trainer.train(model['inputs'], model['targets'], STEPS, npm.optimizer.SGDOptimizer(LR))
    values = _losses(out.getvalue())
    print('losses:', ' '.join(f'{v:.4f}' for v in values))
    assert len(values) == STEPS and np.isfinite(values).all()
    assert all(b < a for a, b in zip(values, values[1:])), values
    with contextlib.redirect_stdout(out):
        trainer.eval(model['inputs'], model['targets'])
    assert _losses(out.getvalue())[-1] < values[-1]
    with pytest.raises(RuntimeError):
        loss_.backward()                                        # eval wrote no gradient

    logits = _teacher_forced_logits(model)
    targets = model['targets'].reshape(B, S)
    top2 = np.sort(logits, axis=-1)[..., -2:]
    live = targets >= 0
    gap = float(((top2[..., 1] - top2[..., 0])[live]).min() / np.abs(logits[live]).max())
    print(f'least top-2 gap of the teacher-forced logits {gap:.3e} of max |logit|')
    assert gap >= GAP, 'a near-tie: incremental decoding and the training forward may pick different tokens'
    learned = [b for b in range(B) if (np.argmax(logits[b], axis=-1) == targets[b])[live[b]].all()]
    print('sequences whose every next token is the argmax after training:', learned)
    assert learned, 'eight steps did not fit any sequence of the batch'
    prompt_len = 2
    generated = _greedy(npm, model, prompt_len, S + 1 - prompt_len)
    same = [b for b in learned if generated[b, :LENGTHS[b] - prompt_len].tolist() == model['tokens'][b, prompt_len:LENGTHS[b]].tolist()]
    print('continued from a prompt of two tokens:', same)
    assert same == learned
