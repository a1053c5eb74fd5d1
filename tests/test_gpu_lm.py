"""GPU: the decoder-only language model ``models.CausalLM`` at the fixture of tests/lm_cases.py -- F 32, 2 heads over 1 key / value
head, hidden 48, vocabulary 50, 3 layers, B 3, S 6, ragged lengths (6, 3, 5); rms + swiglu + rope, and one LayerNorm + ReLU case.

Bounds.
* (1) Logits and every parameter gradient of one training step against the float64 restatement ``lm_cases.reference_step``, at the
  project's parity contract (include/npm_hip.h NPM_PARITY_REL_F32 on the elements of at least 0.1 of the tensor's maximum,
  NPM_PARITY_SCALED_F32 on all) in the form tests/test_gpu_lm_train.py ``_parity`` has.
* (2) ``lm.decode`` in chunks against ``forward``, row for row, within LAYER_TOL = 1e-5 of max |logit| (tests/test_gpu_decode.py);
  an fp16 cache against the model given the fp16-rounded cache rows: the same model decoded in one chunk over an fp16 cache.
* (5) Tokens are compared only after every top-2 logit gap of the teacher-forced run was asserted to be at least
  GAP = 100 LAYER_TOL of max |logit| (tests/test_gpu_spec.py's rule); the seed was chosen on the host simulator
  (tests/test_lm_host.py asserts five times that there).

Every test needs ``models.CausalLM``: none passes on the parent commit."""

import contextlib
import io

import numpy as np
import pytest

import lm_cases as MC

pytestmark = pytest.mark.gpu

STEPS, LR = 8, 0.05                    # plain SGD: see test_eight_sgd_steps_each_lower_the_loss


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


def _parity(got, ref, what):
    from np_modeling_amd import _C
    rel_bound, scaled_bound = _C.parity_bounds()['f32']
    top = np.abs(ref).max()
    err = np.abs(got - ref)
    big = np.abs(ref) >= 0.1 * top
    scaled, rel = float(err.max() / top), float((err[big] / np.abs(ref[big])).max())
    print(f'{what}: rel {rel:.2e} scaled {scaled:.2e}')
    assert scaled <= scaled_bound and rel <= rel_bound, (what, rel, scaled)


def _rows_close(got, want, lengths, tol, what):
    """Rows t < lengths[b] of [B, S, V] within ``tol`` of the largest |logit| of the reference."""
    top = max(float(np.abs(want[b, :n]).max()) for b, n in enumerate(lengths))
    worst = max(float(np.abs(got[b, :n] - want[b, :n]).max()) for b, n in enumerate(lengths))
    print(f'{what}: {worst / top:.2e} of max |logit| (bound {tol:.0e})')
    assert np.isfinite(got).all() and worst <= tol * top, (what, worst / top)


# ---- (1) one training step against float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('keywords', [dict(), dict(norm='layer', ffn='relu')], ids=['rms-swiglu', 'layer-relu'])
def test_logits_and_every_gradient_of_one_step_against_float64(npm, keywords):
    lm = MC.make_lm(npm, **keywords)
    _, inputs, targets = MC.tokens()
    kw = dict(norm='rms', ffn='swiglu')
    kw.update(keywords)
    ref_logits, ref_loss, ref_grads = MC.reference_step(lm, inputs, targets, **kw)
    loss_ = npm.loss.SoftmaxCrossEntropyLoss()
    logits = lm(inputs)
    loss = loss_(logits, targets)
    live = targets >= 0
    _parity(logits.numpy()[live], ref_logits[live], 'logits')
    print(f'loss: ours {loss:.9g} float64 {ref_loss:.9g}')
    from np_modeling_amd import _C
    assert abs(loss - ref_loss) <= _C.parity_bounds()['f32'][0] * abs(ref_loss)
    ours = MC.Recorder()
    assert lm(loss_(backprop=True), backprop=True, optimizer_=ours) is None
    assert ours.grads.keys() == ref_grads.keys()
    for key, want in ref_grads.items():
        got = ours.grads[key]
        # (with the rotation the key bias has a gradient like any other: it is exactly zero only without rope)
        _parity(got, want, f'{key[1]} {got.shape}')
    assert len(lm._causal_mask.masks) == 2 and all(not block._causal_masks for block in lm.layers)       # one mask per (B, S)


# ---- (2) chunked decode equals forward --------------------------------------------------------------------------------------------
def _decode_chunks(lm, inputs, chunks, **start):
    state = lm.start_decoding(MC.B, 8, **start)
    lengths, at, rows = np.array(MC.LENGTHS), 0, []
    for t in chunks:
        n = np.clip(lengths - at, 0, t)
        rows.append(lm.decode(inputs[:, at:at + t], state, new_lengths=n, rows='all').numpy().reshape(MC.B, t, MC.VOCAB))
        at += t
    assert state.positions.tolist() == list(MC.LENGTHS)
    return np.concatenate(rows, axis=1), state


@pytest.mark.parametrize('setting', [dict(), dict(page_size=16), dict(page_size=16, cache_dtype='f16'), dict(window=4)],
                         ids=['f32', 'paged16', 'paged16-f16', 'window4'])
def test_chunked_decode_equals_forward(npm, setting):
    setting = dict(setting)
    lm = MC.make_lm(npm, window=setting.pop('window', None))
    _, inputs, _ = MC.tokens()
    want = lm(inputs).numpy()
    if setting.get('cache_dtype') == 'f16':
        # the model given the fp16-rounded cache rows: one chunk over an fp16 cache (every row attends to the rows as stored)
        plain = want
        want, _ = _decode_chunks(lm, inputs, (6,), **setting)
        top = max(float(np.abs(plain[b, :n]).max()) for b, n in enumerate(MC.LENGTHS))
        print('fp16 cache against forward: %.2e of max |logit| (reported)' %
              (max(float(np.abs(want[b, :n] - plain[b, :n]).max()) for b, n in enumerate(MC.LENGTHS)) / top))
    for chunks in ((6,), (1,) * 6, (2, 1, 3)):
        got, state = _decode_chunks(lm, inputs, chunks, **setting)
        _rows_close(got, want, MC.LENGTHS, MC.LAYER_TOL, f'chunks {chunks} {setting}')
        assert state.self_cache.layers == MC.LAYERS and [block._self_attention._cached_path for block in lm.layers] == ['decode'] * MC.LAYERS
    last = lm.decode(inputs, lm.start_decoding(MC.B, 8, **setting), new_lengths=np.array(MC.LENGTHS)).numpy()
    for b, n in enumerate(MC.LENGTHS):
        assert np.abs(last[b] - want[b, n - 1]).max() <= MC.LAYER_TOL * np.abs(want).max()            # rows='last': row n[b] - 1


# ---- (3) the fused launch is bit-neutral -------------------------------------------------------------------------------------------
def _valid_rows(cache):
    """The valid rows of every K and V tensor of a layered cache, as stored: [(layer, tensor, sequence)] -> array of rows."""
    out = []
    for i in range(cache.layers):
        view = cache.layer(i)
        for x in (view.k.numpy(), view.v.numpy()):
            for b in range(cache.batch):
                rows = range(int(cache.lengths[b]))
                if cache.paged:
                    out.append(np.stack([x[cache.block_table[b, j // cache.page_size], j % cache.page_size] for j in rows]))
                else:
                    out.append(np.stack([x[b, j] for j in rows]))
    return out


@pytest.mark.parametrize('setting', [dict(), dict(page_size=16), dict(page_size=16, cache_dtype='f16')], ids=['f32', 'paged16', 'paged16-f16'])
def test_the_fused_rope_append_switch_changes_no_bit(npm, setting):
    from np_modeling_amd import _C
    lm = MC.make_lm(npm)
    _, inputs, _ = MC.tokens()
    assert lm.fused_rope_append
    runs = {}
    for on in (True, False):
        lm.fused_rope_append = on
        got, state = _decode_chunks(lm, inputs, (2, 1, 3), **setting)
        runs[on] = (got, _valid_rows(state.self_cache))
        if on:
            assert _C.lib().npm_last_rope_append_kernel().decode().startswith('rope_kv_append_kernel D=16 vec=1 rope=1 varlen=1 paged=%d kv=%s' % (
                setting.get('page_size', 0), setting.get('cache_dtype', 'f32')))
    for b, n in enumerate(MC.LENGTHS):
        assert runs[True][0][b, :n].tobytes() == runs[False][0][b, :n].tobytes(), f'the logits of sequence {b} differ'
    assert len(runs[True][1]) == 2 * MC.LAYERS * MC.B
    for a, b in zip(runs[True][1], runs[False][1]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- (4) training -----------------------------------------------------------------------------------------------------------------
def test_eight_sgd_steps_each_lower_the_loss(npm):
    """Plain SGD at 0.05.  On the host simulator every one of the eight steps lowers the loss for rates 0.002 .. 0.15 (at 0.05 by
    0.17 or more each); at 0.2 the eighth step goes up."""
    lm = MC.make_lm(npm)
    _, inputs, targets = MC.tokens()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        npm.train.Trainer([lm], npm.loss.SoftmaxCrossEntropyLoss()).train(inputs, targets, STEPS, npm.optimizer.SGDOptimizer(LR))
    values = [float(line.split()[-1]) for line in out.getvalue().splitlines() if line.startswith('Loss:')]
    print('losses:', ' '.join(f'{v:.4f}' for v in values))
    assert len(values) == STEPS and np.isfinite(values).all()
    assert all(b < a for a, b in zip(values, values[1:])), values


# ---- (5) the generation loops --------------------------------------------------------------------------------------------------------
def test_generate_speculative_and_beam_emit_the_teacher_forced_argmax(npm):
    lm = MC.make_lm(npm)
    emit = 6
    prompt, lengths = MC.prompts(), np.array(MC.PROMPTS)
    generated = lm.generate(prompt, lengths, emit, npm.sampling.Sampler(MC.B))
    # teacher forcing: the prompt and what was generated through forward; position lengths[b] - 1 + i predicts token i
    width = int(lengths.max()) + emit
    full = np.full([MC.B, width], -1, dtype=np.int64)
    for b, n in enumerate(lengths):
        full[b, :n], full[b, n:n + emit] = prompt[b, :n], generated[b]
    logits = lm(full).numpy()
    rows = np.stack([logits[b, n - 1:n - 1 + emit] for b, n in enumerate(lengths)])                   # [B, emit, V]
    gap = MC.top2_gap(rows)
    print(f'least top-2 gap of the teacher-forced logits {gap:.3e} of max |logit| (asked: {MC.GAP:.0e})')
    assert gap >= MC.GAP, 'a fixture error: a near-tie, incremental decoding and the training forward may pick different tokens'
    assert generated.tolist() == rows.argmax(axis=-1).tolist()
    speculative, steps = MC.speculative(npm, lm, emit, page_size=16)
    assert [s[:emit] for s in speculative] == generated.tolist() and steps <= emit
    search, _, seen = MC.beam(npm, lm, MC.B, 1, emit)
    assert len(seen) == emit and [search.hypotheses(g)[0][0] for g in range(MC.B)] == generated.tolist()


# ---- (6) operations on a paged 3-layer state ---------------------------------------------------------------------------------------
def _run(lm, state, steps, ops=()):
    """``steps``: per step the tokens every slot brings; ``ops[i]``: what happens to the state in front of step i.  The last row's
    logits of every slot that brought something, per step."""
    outs = []
    for i, tokens in enumerate(steps):
        for op in ops[i] if i < len(ops) else ():
            op(state)
        n = np.array([len(t) for t in tokens])
        chunk = np.full([4, int(n.max())], -1, dtype=np.int64)
        for b, t in enumerate(tokens):
            chunk[b, :len(t)] = t
        out = lm.decode(chunk, state, new_lengths=n).numpy()
        outs.append({b: out[b] for b in range(4) if n[b]})
    return outs


def test_fork_reorder_release_and_admit_equal_sequences_decoded_on_their_own(npm):
    """One run forks slot 0 into slot 3, swaps slots 0 and 2 and re-admits slot 1; the other feeds every sequence into the slot it
    ends up in, with the same chunk shapes (tests/test_gpu_fork.py's notion of "on their own").  Same kernels, same rows: the same bits."""
    lm = MC.make_lm(npm)
    rng = np.random.default_rng(8)
    s0, s1, s2, s3, y = (rng.integers(0, MC.VOCAB, 12).tolist() for _ in range(5))
    operated = [[s0[:5], s1[:3], s2[:4], []],
                [[s0[5]], [s1[3]], [s2[4]], [s3[0]]],             # behind the fork: slot 3 diverges, copy-on-write in one launch
                [[s0[6]], [s1[4]], [s2[5]], [s3[1]]],
                [[s2[6]], [s1[5]], [s0[7]], [s3[2]]],             # behind the reorder: slots 0 and 2 have swapped
                [[s2[7]], y[:4], [s0[8]], []],                    # behind release + admit: a new sequence in slot 1
                [[s2[8]], [y[4]], [], [s3[3]]]]
    ops = [(), (lambda st: lm.fork(st, 0, 3),), (), (lambda st: lm.reorder(st, [2, 1, 0, 3]),),
           (lambda st: lm.release(st, 1), lambda st: lm.admit(st, 1)), ()]
    own = [[s2[:4], [], s0[:5], s0[:5]],
           [[s2[4]], [], [s0[5]], [s3[0]]],
           [[s2[5]], [], [s0[6]], [s3[1]]],
           [[s2[6]], [], [s0[7]], [s3[2]]],
           [[s2[7]], y[:4], [s0[8]], []],
           [[s2[8]], [y[4]], [], [s3[3]]]]
    where = [{0: 2, 2: 0}, {0: 2, 2: 0, 3: 3}, {0: 2, 2: 0, 3: 3}, {0: 0, 2: 2, 3: 3}, {0: 0, 1: 1, 2: 2}, {0: 0, 1: 1, 3: 3}]
    state = lm.start_decoding(4, 32, page_size=16, pages=10)
    got = _run(lm, state, operated, ops)
    cache = state.self_cache
    assert cache.page_copies == 1 and cache.lengths.tolist() == [9, 5, 9, 9]
    assert cache.pages_in_use == np.unique(cache.block_table[cache.block_table >= 0]).size == 4
    want = _run(lm, lm.start_decoding(4, 32, page_size=16, pages=10), own)
    for step, slots in enumerate(where):
        for a, b in slots.items():
            assert np.array_equal(got[step][a].view(np.uint32), want[step][b].view(np.uint32)), \
                f'step {step}: slot {a} differs from the sequence decoded on its own (slot {b})'
