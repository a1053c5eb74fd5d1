"""CPU: the decoder-only language model on the host simulator (tests/hostsim/; its two fused cache calls join it with the profile 'lm').

* ``TransformerDecoder(cross_attention=False, causal=False)`` IS ``TransformerEncoder``: the same entry points in the same order and
  the same bits, for every norm x feed-forward x norm order, fused and literal; its refusals;
* ``models.CausalLM`` equals its sub-layers chained by hand, logits and gradients, bit for bit, and a float64 restatement;
* a decode step's uploads do not grow with the number of layers; copy-on-write is one launch for all planes;
* every layer view of a layered cache holds what an independent single-layer cache driven the same way holds;
* ``speculative.decode_step`` and ``beam.decode_step`` run the multi-layer model through ``lm.stack`` unchanged;
* the switch of npm_rope_kv_append changes the launches and not one bit;
* header, bindings, Makefile and the built library agree on npm_kv_copy_pages_planes and npm_rope_kv_append.

Every test names ``cross_attention=``, ``models``, ``layers=`` or the new entry point: none passes on the parent commit."""

import ctypes
import os
import re

import numpy as np
import pytest

import llama_cases as LC
import llama_reference as LR
import lm_cases as MC
from hostsim.fixtures import npm_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

npm = npm_fixture()


# ---- cross_attention=False ---------------------------------------------------------------------------------------------------------
def _block_run(npm, kind, norm, ffn, norm_first, literal, **extra):
    """(entry points called, out, dx, parameters after one SGD step) of a seeded layer at tests/llama_cases.py's shape."""
    from np_modeling_amd import device as D, parallel
    np.random.seed(7)
    keywords = dict(num_heads=LC.HEADS, hidden_units=LC.U, norm_first=norm_first, norm=norm, ffn=ffn, **extra)
    if kind == 'encoder':
        layer = npm.layers.TransformerEncoder(**keywords)
    else:
        layer = npm.layers.TransformerDecoder(cross_attention=False, causal=False, **keywords)
    x, dy = LC.inputs(8, [LC.B, LC.S, LC.F], [LC.B, LC.S, LC.F])
    calls = npm.sim.calls
    del calls[:]
    layer(x)
    LC.tame(layer)
    opt = npm.optimizer.SGDOptimizer(0.05)
    if literal:
        out = layer._forward_unfused(D.as_device(x))
        with parallel.grad_scope(layer._numel(), layer._arena) as scope:
            dx = layer._backward_unfused(D.as_device(dy), opt, scope)
    else:
        out = layer(x)
        dx = layer(dy, backprop=True, optimizer_=opt)
    assert not isinstance(dx, tuple)
    return list(calls), np.asarray(out), np.asarray(dx), LR.values(layer), layer


@pytest.mark.parametrize('literal', [False, True], ids=['fused', 'literal'])
@pytest.mark.parametrize('norm_first', [True, False], ids=['pre', 'post'])
@pytest.mark.parametrize('ffn', ['relu', 'swiglu'])
@pytest.mark.parametrize('norm', ['layer', 'rms'])
def test_a_decoder_without_cross_attention_that_is_not_causal_is_the_encoder(npm, norm, ffn, norm_first, literal):
    want = _block_run(npm, 'encoder', norm, ffn, norm_first, literal)
    got = _block_run(npm, 'decoder', norm, ffn, norm_first, literal)
    assert got[0] == want[0] and len(got[0]) > 10
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[3].keys() == want[3].keys() and len(got[3]) == (16 if norm == 'layer' else 14)
    for name in want[3]:
        assert np.array_equal(got[3][name], want[3][name]), name
    layer = got[4]
    assert layer._arena.size == sum(v.size for v in got[3].values()) and layer._numel() == want[4]._numel()
    assert not hasattr(layer, '_cross_attention') and not hasattr(layer, '_norm3') and not hasattr(layer, '_dropout3')


def test_rope_gqa_and_dropout_keep_their_meaning_without_cross_attention(npm):
    extra = dict(rope_base=500.0, num_kv_heads=1)
    want = _block_run(npm, 'encoder', 'rms', 'swiglu', True, False, **extra)
    got = _block_run(npm, 'decoder', 'rms', 'swiglu', True, False, **extra)
    assert got[0] == want[0] and 'npm_rope' in got[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    for kind in ('encoder', 'decoder'):
        run = _block_run(npm, kind, 'layer', 'relu', True, False, drop_rate=0.25)
        assert 'npm_layernorm_dropout_fwd' in run[0]


def test_the_calls_of_a_decoder_without_cross_attention(npm):
    np.random.seed(1)
    dec = npm.layers.TransformerDecoder(num_heads=2, hidden_units=48, norm_first=True, causal=True, cross_attention=False,
                                        norm='rms', ffn='swiglu', rope_base=10000.0)
    x, kv = LC.inputs(2, [2, 8, 32], [2, 6, 32])
    with pytest.raises(TypeError):
        dec(x, kv)
    with pytest.raises(RuntimeError):
        dec.start_decoding(None, 16, batch=2)                     # no parameters yet
    whole = np.asarray(dec(x))
    LC.tame(dec)
    whole = np.asarray(dec(x))
    for bad in (dict(kv=kv, batch=2), dict(kv=None), dict(kv=None, batch=2, kv_lengths=[1, 1]), dict(kv=None, batch=2, memory_capacity=4)):
        with pytest.raises(ValueError):
            dec.start_decoding(bad.pop('kv'), 16, **bad)
    state = dec.start_decoding(None, 16, batch=2, page_size=16, weights='f16')
    assert state.cross_cache is None and len(state.weights._sources) == 6
    state = dec.start_decoding(None, 16, batch=2, page_size=16)
    names = npm.sim.calls
    del names[:]
    rows = [np.asarray(dec.decode(x[:, :5], state)), np.asarray(dec.decode(x[:, 5:6], state))]
    assert names.count('npm_rmsnorm_fwd') == 2 * 2 and names.count('npm_swiglu_fwd') == 2          # two blocks a step
    got = np.concatenate(rows, axis=1)
    np.testing.assert_allclose(got, whole[:, :6], rtol=2e-5, atol=2e-5 * np.abs(whole).max())
    with pytest.raises(ValueError):
        dec.admit(state, 0)                                       # still holds rows
    with pytest.raises(ValueError):
        dec.reorder(state, [0, 1], memory='copy')
    dec.reorder(state, [1, 0])
    state.release(0)
    dec.admit(state, 0)
    with pytest.raises(ValueError):
        dec.admit(state, 0, kv[:1])
    dec.fork(state, 1, 0)
    state.truncate(1)
    assert state.positions.tolist() == [5, 5]
    with pytest.raises(RuntimeError):
        dec(x, backprop=True, optimizer_=None)                    # backward after decode


def test_the_default_decoder_still_wants_its_memory(npm):
    dec = npm.layers.TransformerDecoder(num_heads=2, hidden_units=48, norm_first=True, causal=True)
    x, kv = LC.inputs(2, [2, 8, 32], [2, 6, 32])
    with pytest.raises(TypeError):
        dec(x)
    dec(x, kv)
    assert isinstance(dec(x, backprop=True, optimizer_=MC.Recorder()), tuple) and len(LR.parameters(dec)) == 26
    with pytest.raises(ValueError):
        dec.start_decoding(kv, 16, batch=2)
    with pytest.raises(TypeError):
        dec.admit(dec.start_decoding(kv, 16), 0)


# ---- CausalLM ------------------------------------------------------------------------------------------------------------------------
KINDS = [dict(), dict(norm='layer', ffn='relu'), dict(norm_first=False), dict(window=4)]


def _by_hand(npm, keywords):
    """The sub-layers of ``make_lm`` drawn from the same seed in the same order, chained by hand."""
    from np_modeling_amd.layers import transformer
    np.random.seed(MC.SEED)
    kw = dict(norm='rms', ffn='swiglu', norm_first=True, window=None)
    kw.update(keywords)
    norm_first = kw.pop('norm_first')
    emb = npm.layers.Embedding(MC.VOCAB, MC.F)
    blocks = [npm.layers.TransformerDecoder(MC.HEADS, MC.HIDDEN, norm_first, num_kv_heads=MC.HKV, causal=True, rope_base=MC.ROPE_BASE,
                                            cross_attention=False, **kw) for _ in range(MC.LAYERS)]
    final = transformer._make_norm(kw['norm'], None) if norm_first else None
    head = npm.layers.Linear(units=MC.VOCAB)

    def forward(ids):
        x = emb(ids)
        for block in blocks:
            x = block(x)
        if final is not None:
            x = final(x)
        return head(x.reshape(-1, MC.F))

    def backward(dlogits, opt):
        dx = head(dlogits, backprop=True, optimizer_=opt).reshape(MC.B, -1, MC.F)
        if final is not None:
            dx = final(dx, backprop=True, optimizer_=opt)
        for block in blocks[::-1]:
            dx = block(dx, backprop=True, optimizer_=opt)
        emb(dx, backprop=True, optimizer_=opt)

    forward(np.zeros([MC.B, 2], dtype=np.int64))
    for block in blocks:
        for owner, attribute in LR.parameters(block).values():
            value = owner._param(attribute)
            if value.ndim > 1:
                value.set(np.asarray(value) * np.float32(2.0 / np.sqrt(MC.F)))
    head._w.set(np.asarray(head._w) * np.float32(2.0 / np.sqrt(MC.F)))
    return forward, backward, blocks


@pytest.mark.parametrize('keywords', KINDS, ids=['rms-swiglu', 'layer-relu', 'post', 'window4'])
def test_causal_lm_equals_its_layers_chained_by_hand_and_float64(npm, keywords):
    from np_modeling_amd import device as D
    lm = MC.make_lm(npm, **keywords)
    forward, backward, blocks = _by_hand(npm, keywords)
    _, inputs, targets = MC.tokens()
    logits = lm(inputs)
    assert logits.shape == (MC.B, MC.S, MC.VOCAB)
    assert np.array_equal(np.asarray(logits).reshape(-1, MC.VOCAB), np.asarray(forward(inputs)))
    assert len(lm._causal_mask.masks) == 2 and all(not block._causal_masks for block in lm.layers)      # (B, 2) of the draw and (B, S): one each
    assert all(len(block._causal_masks) == 2 for block in blocks)
    assert len({id(block._self_attention._rope) for block in lm.layers}) == 1
    loss_ = npm.loss.SoftmaxCrossEntropyLoss()
    loss = loss_(logits, targets)
    dlogits = loss_(backprop=True)
    ours, theirs = MC.Recorder(), MC.Recorder()
    assert lm(dlogits, backprop=True, optimizer_=ours) is None
    backward(D.as_device(np.asarray(dlogits).reshape(-1, MC.VOCAB)), theirs)
    assert ours.order == theirs.order and len(ours.order) == len(ours.grads)
    assert len(ours.order) == 2 + 1 + MC.LAYERS * len(LR.parameters(lm.layers[0])) + (len(lm.final_norm._segments()) if lm.final_norm else 0)
    for got, want in zip(ours.grads.values(), theirs.grads.values()):
        assert np.array_equal(got, want)
    # float64: the simulator computes in float64 and stores float32
    kw = dict(norm='rms', ffn='swiglu', norm_first=True, window=None)
    kw.update(keywords)
    ref_logits, ref_loss, ref_grads = MC.reference_step(lm, inputs, targets, **kw)
    live = targets >= 0
    np.testing.assert_allclose(np.asarray(logits)[live], ref_logits[live], rtol=2e-4, atol=2e-5 * np.abs(ref_logits[live]).max())
    assert abs(loss - ref_loss) <= 1e-5 * ref_loss
    assert ours.grads.keys() == ref_grads.keys()
    for key, want in ref_grads.items():
        np.testing.assert_allclose(ours.grads[key], want, rtol=0, atol=3e-5 * max(np.abs(want).max(), 1e-3), err_msg=str(key[1]))


def test_trainer_trains_the_model_from_ids_without_an_adapter(npm, capsys):
    lm = MC.make_lm(npm)
    _, inputs, targets = MC.tokens()
    npm.train.Trainer([lm], npm.loss.SoftmaxCrossEntropyLoss()).train(inputs, targets, 3, npm.optimizer.SGDOptimizer(0.02))
    losses = [float(line.split()[-1]) for line in capsys.readouterr().out.splitlines() if line.startswith('Loss:')]
    assert len(losses) == 3 and losses[2] < losses[1] < losses[0]
    assert len(npm.sim.uploads) and isinstance(lm.resident_inputs(inputs), npm.device.IdBuffer)


@pytest.mark.parametrize('setting', [dict(), dict(page_size=16), dict(page_size=16, cache_dtype='f16'), dict(window=4), dict(weights='f16')],
                         ids=['f32', 'paged', 'paged-f16', 'window4', 'w16'])
@pytest.mark.parametrize('chunks', [(6,), (1,) * 6, (2, 1, 3)], ids=['6', '1x6', '2-1-3'])
def test_chunked_decode_equals_forward(npm, setting, chunks):
    setting = dict(setting)
    window = setting.pop('window', None)
    lm = MC.make_lm(npm, window=window)
    _, inputs, _ = MC.tokens()
    whole = np.asarray(lm(inputs))
    state = lm.start_decoding(MC.B, 8, **setting)
    assert state.self_cache.layers == MC.LAYERS and len(state.layers) == MC.LAYERS and state.self_cache.nbytes == \
        2 * MC.LAYERS * state.self_cache.k.nbytes
    lengths, at, rows = np.array(MC.LENGTHS), 0, []
    for t in chunks:
        n = np.clip(lengths - at, 0, t)
        rows.append(np.asarray(lm.decode(inputs[:, at:at + t], state, new_lengths=n, rows='all')).reshape(MC.B, t, MC.VOCAB))
        last = np.asarray(lm.decode(np.zeros([MC.B, 1], dtype=np.int64), state, new_lengths=np.zeros(MC.B, dtype=np.int64)))
        assert last.shape == (MC.B, MC.VOCAB) and (last == last[0]).all()                   # nobody brought a row: the zero row's logits
        at += t
    got = np.concatenate(rows, axis=1)
    assert state.positions.tolist() == list(MC.LENGTHS)
    tol = 2e-2 if 'f16' in setting.values() else 2e-5
    for b, n in enumerate(MC.LENGTHS):
        np.testing.assert_allclose(got[b, :n], whole[b, :n], rtol=tol, atol=tol * np.abs(whole).max())
    with pytest.raises(ValueError):
        lm.decode(inputs[:, :3], state, rows='some')
    with pytest.raises(ValueError):
        lm.decode(inputs[:, :4], state)                            # 4 more rows do not fit 8: refused with nothing changed
    assert state.self_cache._step is None and state.positions.tolist() == list(MC.LENGTHS)


# ---- one set of cache state ------------------------------------------------------------------------------------------------------------
def _six_steps(npm, layers):
    """Six decode steps on a paged ragged batch of four slots with a fork, a release + admit and a truncate between them."""
    lm = MC.make_lm(npm, layers=layers)
    rng = np.random.default_rng(5)
    state = lm.start_decoding(4, 32, page_size=16, pages=12)
    cache, sim = state.self_cache, npm.sim
    del sim.calls[:]
    log = []

    def step(tokens, n):
        uploads, table, calls = len(sim.uploads), cache.table_uploads, len(sim.calls)
        lm.decode(rng.integers(0, MC.VOCAB, [4, tokens]), state, new_lengths=np.array(n))
        names = sim.calls[calls:]
        log.append(dict(uploads=sim.uploads[uploads:], table=cache.table_uploads - table, planes=names.count('npm_kv_copy_pages_planes'),
                        single=names.count('npm_kv_copy_pages'), appends=names.count('npm_kv_append_paged'),
                        fused=names.count('npm_rope_kv_append'), ropes=names.count('npm_rope')))

    step(5, [5, 3, 4, 0])
    lm.fork(state, 0, 3)
    step(1, [1, 1, 1, 1])                    # slots 0 and 3 share a partly filled page: one of them copies it
    step(2, [2, 2, 2, 2])
    state.truncate(np.array([1, 0, 1, 0]))
    lm.release(state, 1)
    lm.admit(state, 1)
    step(3, [1, 3, 1, 1])
    lm.reorder(state, [0, 1, 3, 2])
    step(1, [1, 1, 1, 1])
    step(1, [1, 0, 1, 1])
    return log, cache, state


def test_uploads_do_not_grow_with_the_number_of_layers(npm):
    one, cache1, _ = _six_steps(npm, 1)
    three, cache3, state = _six_steps(npm, 3)
    assert [s['uploads'] for s in one] == [s['uploads'] for s in three]              # count and bytes, step by step
    assert sum(len(s['uploads']) for s in three) > 0
    for cache, steps in ((cache1, one), (cache3, three)):
        assert all(s['table'] <= 1 for s in steps) and cache.table_uploads <= len(steps)
    assert cache1.lengths.tolist() == cache3.lengths.tolist() == [10, 4, 11, 9]
    assert np.array_equal(cache1.block_table, cache3.block_table) and np.array_equal(cache1.refcount, cache3.refcount)
    # copy-on-write: one launch for K and V of every layer in a step that copies, never the single-tensor call
    assert [s['planes'] for s in three] == [0, 1, 0, 0, 0, 0] and not any(s['single'] for s in three)
    assert npm.sim.plane_calls == [(1, 6)] and cache3.page_copies == 1 == cache1.page_copies
    assert [s['single'] for s in one] == [0, 2, 0, 0, 0, 0] and not any(s['planes'] for s in one)      # one layer: the cache as it was
    # the model turns the fused launch on for its layers: one per layer and step in place of npm_rope and two appends
    assert [s['fused'] for s in three] == [3] * 6 and [s['fused'] for s in one] == [1] * 6
    assert not any(s['appends'] or s['ropes'] for s in one + three)
    assert state.self_cache is cache3 and cache3._step is None


@pytest.mark.parametrize('setting', [dict(), dict(dtype='f16'), dict(page_size=16), dict(page_size=16, dtype='f16'),
                                     dict(page_size=16, window=5), dict(window=5)],
                         ids=['f32', 'f16', 'paged', 'paged-f16', 'paged-window5', 'window5'])
def test_layer_views_hold_what_independent_caches_hold(npm, setting):
    D = npm.device
    hkv, d, n_layers, batch, capacity = 2, 16, 3, 4, 48
    row = hkv * d
    paged = 'page_size' in setting
    make = (lambda **kw: D.PagedKVCache(batch, capacity, hkv, d, pages=14, **setting, **kw)) if paged else \
        (lambda **kw: D.KVCache(batch, capacity, hkv, d, **setting, **kw))
    layered, alone = make(layers=n_layers), [make() for _ in range(n_layers)]
    assert layered.layers == n_layers and layered.nbytes == sum(c.nbytes for c in alone)
    rng = np.random.default_rng(9)

    def step(tokens, n):
        k, v = (rng.standard_normal([n_layers, batch, tokens, row]).astype(np.float32) for _ in range(2))
        lens = None if n is None else np.array(n)
        layered.begin(tokens, lens)
        for i in range(n_layers):
            kd, vd = D.from_host(k[i]), D.from_host(v[i])
            view = layered.layer(i)
            view.room(tokens, lens)
            view.append(D.Mat(kd, row), D.Mat(vd, row), tokens, lens)
            alone[i].append(D.Mat(kd, row), D.Mat(vd, row), tokens, lens)
            assert view.lengths.tolist() == alone[i].lengths.tolist() and view.max_length == alone[i].max_length
            assert view.ragged == alone[i].ragged
        layered.commit()

    def same():
        for i, single in enumerate(alone):
            view = layered.layer(i)
            assert layered.lengths.tolist() == single.lengths.tolist()
            for mine, theirs in ((view.k, single.k), (view.v, single.v)):
                got, want = mine.numpy(), theirs.numpy()
                assert got.dtype == want.dtype and got.shape == want.shape
                for b in range(batch):
                    first = int(layered.dropped[b]) if paged else 0
                    for j in range(first, int(layered.lengths[b])):
                        if paged:
                            page = layered.block_table[b, j // 16]
                            assert page == single.block_table[b, j // 16] and page >= 0
                            assert np.array_equal(got[page, j % 16], want[page, j % 16]), (i, b, j)
                        else:
                            assert np.array_equal(got[b, j], want[b, j]), (i, b, j)
            if paged:
                assert np.array_equal(layered.refcount, single.refcount) and sorted(layered._free) == sorted(single._free)
                assert layered.dropped.tolist() == single.dropped.tolist() and layered.page_copies == single.page_copies

    def both(op, *args):
        for cache in [layered] + alone:
            getattr(cache, op)(*args)

    step(3, None)                                # uniform: the scalar call on a contiguous cache
    same()
    step(14, [14, 3, 11, 0])                     # a chunk that crosses a 16-row page
    same()
    if paged:
        both('release', 3)                       # a paged fork wants an empty slot; a contiguous one overwrites
    both('fork', 0, 3)
    step(2, [2, 1, 0, 2])                        # the fork's copy-on-write
    same()
    both('truncate', np.array([1, 0, 2, 1]))
    both('reorder', [2, 1, 0, 3])
    step(1, None)
    same()
    if paged:
        both('release', 1)
        step(20, [1, 20, 1, 1])
        same()
        assert layered.table_uploads == alone[0].table_uploads
    with pytest.raises(ValueError):
        layered.append(None, None, 1)
    with pytest.raises(RuntimeError):
        layered.layer(0).append(None, None, 1)               # no step is open
    with pytest.raises(ValueError):
        layered.begin(capacity, None)
    assert layered._step is None


def test_a_layered_cache_refuses_what_it_cannot_hold(npm):
    D = npm.device
    with pytest.raises(ValueError, match='head sizes'):
        D.KVCache(2, 8, 2, 16, 8, layers=2)
    with pytest.raises(ValueError, match='layers'):
        D.PagedKVCache(2, 8, 2, 16, page_size=16, layers=0)
    plain = D.KVCache(2, 8, 2, 16)
    assert plain.layers == 1 and plain._planes is None
    cache = D.KVCache(2, 8, 2, 16, layers=2)
    cache.begin(1)
    with pytest.raises(RuntimeError):
        cache.begin(1)
    with pytest.raises(ValueError):
        cache.layer(0).room(2)                                # not what begin() was told
    cache.commit()
    with pytest.raises(RuntimeError):
        cache.commit()
    assert cache.lengths.tolist() == [1, 1]


# ---- npm_rope_kv_append: the switch -----------------------------------------------------------------------------------------------------
def _planes(cache):
    return [cache.layer(i).k.numpy() for i in range(cache.layers)] + [cache.layer(i).v.numpy() for i in range(cache.layers)]


@pytest.mark.parametrize('setting', [dict(), dict(page_size=16), dict(page_size=16, cache_dtype='f16'), dict(cache_dtype='f16'),
                                     dict(rope_base=None), dict(window=4, page_size=16)],
                         ids=['f32', 'paged', 'paged-f16', 'f16', 'no-rope', 'window4-paged'])
def test_the_fused_switch_changes_the_launches_and_not_one_bit(npm, setting):
    setting = dict(setting)
    model = {k: setting.pop(k) for k in ('rope_base', 'window') if k in setting}
    lm = MC.make_lm(npm, **model)
    _, inputs, _ = MC.tokens()
    assert lm.fused_rope_append and not npm.device.FUSED_ROPE_APPEND              # the model's own choice; the module's is off
    runs = {}
    for on in (True, False):
        lm.fused_rope_append = on
        state = lm.start_decoding(MC.B, 8, **setting)
        names = npm.sim.calls
        del names[:]
        out = [np.asarray(lm.decode(inputs[:, :3], state, new_lengths=np.array([3, 3, 3]))),              # uniform from empty
               np.asarray(lm.decode(inputs[:, 3:5], state, new_lengths=np.array([2, 0, 2]), rows='all')),  # ragged
               np.asarray(lm.decode(inputs[:, 5:6], state, new_lengths=np.array([1, 0, 0])))]
        rope = 0 if model.get('rope_base', 1) is None else 1
        if on:
            assert names.count('npm_rope_kv_append') == 3 * MC.LAYERS and 'npm_rope' not in names
            assert not [n for n in names if n.startswith('npm_kv_append')]
            assert all(c['rope'] == bool(rope) and c['f16'] == (setting.get('cache_dtype') == 'f16') for c in npm.sim.fused_calls)
            assert npm.sim.npm_last_rope_append_kernel().decode().startswith('rope_kv_append_kernel D=16 vec=1 rope=%d varlen=1' % rope)
        else:
            assert 'npm_rope_kv_append' not in names and names.count('npm_rope') == 3 * MC.LAYERS * rope
            assert len([n for n in names if n.startswith('npm_kv_append')]) == 2 * 3 * MC.LAYERS
        runs[on] = (out, _planes(state.self_cache), state.positions.tolist())
    assert runs[True][2] == runs[False][2] == [6, 3, 5]
    for a, b in zip(runs[True][0] + runs[True][1], runs[False][0] + runs[False][1]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()                  # raw bits: unwritten cache rows are NaN in both


def test_the_module_switch_routes_a_plain_attention_layer_and_unpacked_parameters_keep_three_launches(npm, monkeypatch):
    import decode_cases as DC
    D = npm.device
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=3, batch=2)
    x = np.random.default_rng(2).standard_normal([2, 5, 64]).astype(np.float32)

    def run():
        cache = att.make_cache(2, 8)
        names = npm.sim.calls
        del names[:]
        outs = [np.asarray(att(x[:, :3], cache=cache)), np.asarray(att(x[:, 3:], cache=cache, new_lengths=[2, 1]))]
        return outs, [n for n in names if n.startswith(('npm_rope', 'npm_kv_append'))], cache.k.numpy(), cache.v.numpy()

    off = run()
    assert off[1] == ['npm_kv_append', 'npm_kv_append', 'npm_kv_append_varlen', 'npm_kv_append_varlen']
    monkeypatch.setattr(D, 'FUSED_ROPE_APPEND', True)
    on = run()
    assert on[1] == ['npm_rope_kv_append'] * 2 and not npm.sim.fused_calls[-1]['rope']
    for a, b in zip(off[0] + list(off[2:]), on[0] + list(on[2:])):
        assert a.tobytes() == b.tobytes()
    att._wk = np.asarray(att._wk).copy()                       # rebound: the projection is three GEMMs, the step three launches
    assert run()[1] == off[1]
    att._fused_rope_append = False                             # a layer's own choice beats the module's
    assert run()[1] == off[1]


# ---- the generation loops, unchanged ---------------------------------------------------------------------------------------------------
def test_the_fixture_has_the_gap_the_gpu_test_asks_for(npm):
    lm = MC.make_lm(npm)
    _, seen, _ = MC.greedy(npm, lm, 6)
    gap = min(MC.top2_gap(z) for z in seen)
    print(f'least top-2 gap of the greedy run {gap:.3e} of max |logit| (the GPU test asks for {MC.GAP:.0e})')
    assert gap >= 5 * MC.GAP


@pytest.mark.parametrize('setting', [dict(page_size=16), dict(page_size=16, cache_dtype='f16'), dict()], ids=['paged', 'paged-f16', 'f32'])
def test_speculative_decode_step_over_the_stack_emits_the_greedy_tokens(npm, setting):
    lm = MC.make_lm(npm)
    want, _, _ = MC.greedy(npm, lm, 6, **setting)
    got, steps = MC.speculative(npm, lm, 6, **setting)
    assert [g[:6] for g in got] == want.tolist() and steps <= 6
    generated = lm.generate(MC.prompts(), MC.PROMPTS, 6, npm.sampling.Sampler(MC.B))
    assert generated.shape == (MC.B, 6) and generated.tolist() == want.tolist()


def test_beam_decode_step_over_the_stack(npm):
    lm = MC.make_lm(npm)
    greedy, _, _ = MC.greedy(npm, lm, 5, page_size=16)
    search, _, seen = MC.beam(npm, lm, 3, 1, 5)
    assert len(seen) == 5
    for g in range(3):
        (tokens, score), = search.hypotheses(g)
        assert tokens == greedy[g].tolist() and np.isfinite(score)
    search, reference, seen = MC.beam(npm, lm, 2, 3, 5)
    for g in range(2):
        got, want = search.hypotheses(g), reference.hypotheses(g)
        assert [t for t, _ in got] == [t for t, _ in want] and len(got) == 3
        assert np.allclose([s for _, s in got], [s for _, s in want], rtol=0, atol=1e-4)


# ---- the entry point -----------------------------------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_declared_bound_and_exported():
    from np_modeling_amd import _C
    text = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    assert re.search(r'#define\s+NPM_ABI_VERSION\s+2\b', text)              # an addition: the version stays
    ctype = {'const int32_t *': ctypes.c_void_p, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'void *': ctypes.c_void_p}
    protos = {}
    for name in ('npm_kv_copy_pages', 'npm_kv_copy_pages_planes'):
        proto = re.search(r'int %s\((.*?)\);' % name, text, flags=re.S).group(1)
        protos[name] = [ctype[re.sub(r'\s*\w+$', '', a.strip()).strip()] for a in proto.split(',')]
    assert protos['npm_kv_copy_pages_planes'] == protos['npm_kv_copy_pages'] + [ctypes.c_int32, ctypes.c_int64]
    assert _C.SIGNATURES['npm_kv_copy_pages_planes'] == protos['npm_kv_copy_pages_planes']
    assert 'npm_kv_copy_pages_planes' not in _C._SPECIAL                 # it returns a status: SIGNATURES, like every such call
    ctype.update({'float *': ctypes.c_void_p, 'const float *': ctypes.c_void_p})
    proto = re.search(r'int npm_rope_kv_append\((.*?)\);', text, flags=re.S).group(1)
    args = [ctype[re.sub(r'\s*\w+$', '', a.strip()).strip()] for a in proto.split(',')]
    assert len(args) == 21 and _C.SIGNATURES['npm_rope_kv_append'] == args and 'npm_rope_kv_append' not in _C._SPECIAL
    assert re.search(r'const char \*npm_last_rope_append_kernel\(void\);', text)
    assert _C._SPECIAL['npm_last_rope_append_kernel'] == (ctypes.c_char_p, [])
    makefile = open(os.path.join(ROOT, 'np_modeling_amd', 'csrc', 'Makefile')).read()
    assert 'npm_rope_append.hip' in re.search(r'SRCS\s*:=(.*)', makefile).group(1)
    if not os.path.exists(_C.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    bound = _C.load_library()
    count = ctypes.c_int(0)
    bound.npm_device_count(ctypes.byref(count))
    assert isinstance(bound.npm_last_rope_append_kernel(), bytes)
    if count.value == 0:
        assert bound.npm_kv_copy_pages_planes(None, 0, 0, None, None, None, 0, 0, 0) == 10001
        assert bound.npm_rope_kv_append(None, 0, 0, 0, 1, 1, 2, None, None, 0, 0, None, None, None, None, 0, 0, None, 0, 0, 0) == 10001
