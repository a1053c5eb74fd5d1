"""CPU: token generation without a GPU, on the simulator of tests/hostsim/ (profile 'sample').

* ``sampling.Sampler`` bookkeeping: counters advance for active rows only, ``set`` restarts a slot, the host mirror equals the
  device vector, the argument checks raise;
* ``layers.Embedding`` forward and backward through the simulator against ``np.add.at`` in float64 at 1e-6, and one SGD step;
* the properties of the case lists of tests/sample_cases.py that tests/test_gpu_sample.py relies on, checked on
  tests/sample_reference.py alone: the exact rows are exact, and in every family of general rows at most 5 % of the (row, draw)
  pairs admit more than one token or more than one ``kept`` within the bound;
* the entry points: header against bindings and exports.

Every test needs ``np_modeling_amd.sampling``, ``layers.Embedding``, ``device.take_rows`` or the new symbols of the library, none of
which exists on the parent commit.
"""

import ctypes

import numpy as np
import pytest

from hostsim.fixtures import npm_fixture
import sample_cases as SC
import sample_reference as SR


npm = npm_fixture('sample')


# ---- Sampler -------------------------------------------------------------------------------------------------------------------------
def test_counters_advance_for_active_rows_only_and_set_restarts_a_slot(npm):
    from np_modeling_amd import device as D
    sampler = npm.sampling.Sampler(3)
    for b in range(3):
        sampler.set(b, temperature=0.8, top_k=5, top_p=0.9, seed=7 + b)
    logits = D.from_host(np.random.default_rng(0).standard_normal([3, 40]).astype(np.float32))
    first = sampler(logits)
    assert sampler.draw.tolist() == [1, 1, 1] and sampler.device_draw().tolist() == [1, 1, 1]
    assert first.numpy().dtype == np.int32 and ((first.numpy() >= 0) & (first.numpy() < 40)).all()
    assert (first.kept >= 1).all() and (first.kept <= 5).all() and ((first.prob > 0) & (first.prob <= 1)).all()
    assert first.ids.shape == (3,) and np.array_equal(first.ids.numpy(), first.numpy())
    second = sampler(logits, active=np.array([1, 0, 2]))
    assert second.numpy()[1] == -1 and second.kept[1] == 0 and second.prob[1] == 0
    assert sampler.draw.tolist() == [2, 1, 2] and sampler.device_draw().tolist() == [2, 1, 2]
    sampler.set(0, temperature=0.8, top_k=5, top_p=0.9, seed=7)
    assert sampler.draw.tolist() == [0, 1, 2] and sampler.device_draw().tolist() == [0, 1, 2]
    again = sampler(logits)
    assert again.numpy()[0] == first.numpy()[0]                       # slot 0: the same seed at counter 0 again
    assert sampler.device_draw().tolist() == sampler.draw.tolist() == [1, 2, 3]
    assert npm.sim.samples[-1]['active'] == 0 and npm.sim.samples[1]['active'] != 0
    assert npm.sim.calls.count('npm_sample_rows') == 3


def test_a_slot_never_set_is_greedy(npm):
    from np_modeling_amd import device as D
    x = np.random.default_rng(1).standard_normal([2, 17]).astype(np.float32)
    out = npm.sampling.Sampler(2)(D.from_host(x))
    assert out.numpy().tolist() == x.argmax(axis=1).tolist() and out.kept.tolist() == [1, 1] and out.prob.tolist() == [1, 1]


@pytest.mark.parametrize('kwargs', [dict(temperature=-0.1), dict(temperature=float('nan')), dict(temperature=float('inf')),
                                    dict(top_k=1.5), dict(top_k=2 ** 31), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float('nan')),
                                    dict(top_p=1e-60), dict(seed=-1), dict(seed=2 ** 64), dict(seed=0.5)])
def test_set_checks_its_arguments(npm, kwargs):
    sampler = npm.sampling.Sampler(2)
    sampler.set(1, temperature=0.5, top_k=3, top_p=0.5, seed=9)
    with pytest.raises(ValueError):
        sampler.set(1, **kwargs)
    assert (sampler.temperature[1], sampler.top_k[1], sampler.top_p[1], sampler.seed[1]) == (0.5, 3, 0.5, 9)      # nothing changed


def test_sampler_checks_its_call(npm):
    from np_modeling_amd import device as D
    with pytest.raises(ValueError):
        npm.sampling.Sampler(0)
    sampler = npm.sampling.Sampler(2)
    for slot in (-1, 2, 0.5):
        with pytest.raises(ValueError):
            sampler.set(slot)
    with pytest.raises(ValueError):
        sampler(np.zeros([2, 5], dtype=np.float32))                   # host logits: the sampler reads device rows
    with pytest.raises(ValueError):
        sampler(D.zeros([3, 5]))
    with pytest.raises(ValueError):
        sampler(D.zeros([2, 5]), active=[1, 1, 1])
    with pytest.raises(ValueError):
        sampler(D.zeros([2, 5]), active=[0.5, 1.0])
    assert 'npm_sample_rows' not in npm.sim.calls


def test_the_simulated_entry_point_refuses_bad_arguments(npm):
    from np_modeling_amd import _C
    lib = _C.lib()
    assert lib.npm_sample_rows(ctypes.byref(_C.npm_sample(batch=1, vocab=4, pitch=4))) == 10002
    buf = np.zeros(16, dtype=np.float32).ctypes.data
    full = dict(logits=buf, temperature=buf, top_k=buf, top_p=buf, seed=buf, draw=buf, token=buf)
    assert lib.npm_sample_rows(ctypes.byref(_C.npm_sample(batch=1, vocab=4, pitch=3, **full))) == 10002
    assert lib.npm_sample_rows(ctypes.byref(_C.npm_sample(batch=1, vocab=(1 << 20) + 1, pitch=1 << 21, **full))) == 10002
    assert lib.npm_sample_rows(ctypes.byref(_C.npm_sample(batch=0, vocab=4, pitch=4, **full))) == 10002


# ---- take_rows and Embedding --------------------------------------------------------------------------------------------------------
def test_take_rows_zero_fills_what_lies_outside(npm):
    from np_modeling_amd import device as D
    table = np.random.default_rng(2).standard_normal([6, 5]).astype(np.float32)
    idx = np.array([[0, 5, -1], [6, 2, 2]])
    got = D.take_rows(D.from_host(table), idx).numpy()
    want = np.where(((idx >= 0) & (idx < 6))[..., None], table[np.clip(idx, 0, 5)], 0)
    assert got.shape == (2, 3, 5) and np.array_equal(got, want)
    on_device = D.ids_from_host(idx)
    assert np.array_equal(D.take_rows(D.from_host(table), on_device).numpy(), want)
    with pytest.raises(ValueError):
        D.take_rows(D.from_host(table), np.array([0.5]))
    with pytest.raises(ValueError):
        D.take_rows(D.zeros([2, 3, 4]), [0])


@pytest.mark.parametrize('ids', [[3, 3, 3, 0, 7, 3], [[1, 2], [2, 9]], [-1, 4, 10, 4]])
def test_embedding_forward_and_backward_against_float64(npm, ids):
    np.random.seed(3)
    emb = npm.layers.Embedding(10, 6)
    y = emb(np.array(ids))
    table = emb.w.numpy()
    idx = np.array(ids)
    inside = (idx >= 0) & (idx < 10)
    assert np.array_equal(y.numpy(), np.where(inside[..., None], table[np.clip(idx, 0, 9)], 0))
    dy = np.random.default_rng(4).standard_normal(idx.shape + (6,)).astype(np.float32)
    want = np.zeros([10, 6])
    np.add.at(want, idx[inside], dy[inside].astype(np.float64))
    lr = 0.25
    assert emb(dy, backprop=True, learning_rate=lr) is None
    np.testing.assert_allclose(emb.w.numpy(), table - lr * want, rtol=0, atol=1e-6 * (1 + np.abs(want).max()))
    assert npm.sim.calls.count('npm_embedding_bwd') == 1 and npm.sim.calls.count('npm_take_rows') == 1
    untouched = np.setdiff1d(np.arange(10), idx[inside])
    assert np.array_equal(emb.w.numpy()[untouched], table[untouched])                 # tokens that did not occur: a zero gradient


def test_embedding_takes_device_ids_and_adam(npm):
    np.random.seed(5)
    sampler = npm.sampling.Sampler(2)
    logits = npm.device.from_host(np.array([[0, 3, 1, 0], [5, 0, 0, 0]], dtype=np.float32))
    result = sampler(logits)
    emb = npm.layers.Embedding(4, 3)
    y = emb(result.ids)
    table = emb.w.numpy()
    assert np.array_equal(y.numpy(), table[[1, 0]])
    emb(np.ones([2, 3], dtype=np.float32), backprop=True, optimizer_=npm.optimizer.AdamOptimizer(0.1))
    moved = emb.w.numpy() != table
    assert moved[[0, 1]].all() and not moved[[2, 3]].any()           # Adam moves a parameter with a zero gradient by 0


# ---- the case lists --------------------------------------------------------------------------------------------------------------------
def test_the_exact_rows_are_exact_and_cover_what_the_gpu_test_says():
    assert set(SC.EXACT_VOCABS) >= {1, 2, 63, 64, 65, 255, 1000, 4099, SC.LDS_ROW - 1, SC.LDS_ROW + 1, 65537}
    from np_modeling_amd import _C
    assert SC.LDS_ROW == _C.SAMPLE_LDS_ROW
    for vocab in SC.EXACT_VOCABS:
        rows = SC.exact_rows(vocab)
        params = SC.exact_params(vocab)
        assert len(params) == 1 + 3 * 6 * 4
        for t in (0.5, 1.0, 3.0):
            for z in rows:
                w = SR.exact_weights(z, t)                             # asserts exactness
                assert w.max() == SR.ONE
        if vocab >= 63:
            assert (rows[:3] == SC.C_LOGIT).any(axis=1).all() and (rows[2] == SC.C_LOGIT).sum() == 1
            assert (rows[0] == -np.inf).any() and (rows[3] == SC.LOW_LOGIT).any()
    # ties at both cuts, broken by index: top-k 2 of a row of many equal c keeps the two lowest indices of them
    z = SC.exact_rows(1000)[1]
    row = SR.ExactRow(z, 1.0, 2, 1.0)
    assert row.k2.tolist() == np.flatnonzero(z == SC.C_LOGIT)[:2].tolist()
    row = SR.ExactRow(z, 1.0, 0, 0.25)
    assert row.kept == -(-int((z == SC.C_LOGIT).sum()) // 4) and row.k2.tolist() == np.flatnonzero(z == SC.C_LOGIT)[:row.kept].tolist()
    # -200 tokens count toward top-k and are never drawn
    z = SC.exact_rows(1000)[2]
    row = SR.ExactRow(z, 1.0, 5, 1.0)
    assert row.kept == 5 and {row.draw(3, d)[0] for d in range(32)} == {int(np.flatnonzero(z == SC.C_LOGIT)[0])}


def test_the_reference_models_agree_on_exact_rows():
    z = SC.exact_rows(255)[0]
    for t, k, p in [(1.0, 0, 1.0), (0.5, 5, 0.5), (3.0, 0, 0.25)]:
        exact, model = SR.ExactRow(z, t, k, p), SR.Float64Row(z, t, k, p)
        assert model.kept_set(SC.EPS) == [exact.kept] or exact.kept in model.kept_set(SC.EPS)
        for d in range(8):
            token = exact.draw(5, d)[0]
            assert token in model.token_set(exact.kept, SR.u24_of(5, d) / 2.0 ** 24, SC.EPS)


def test_at_most_five_percent_of_the_general_pairs_are_ambiguous():
    """The condition tests/test_gpu_sample.py (d) puts on its inputs, from the reference alone."""
    for vocab in SC.GENERAL_VOCABS:
        rows = SC.general_rows(vocab)
        for t, k, p in SC.GENERAL_FAMILIES:
            ambiguous = 0
            for z, seed in zip(rows, SC.GENERAL_SEEDS):
                model = SR.Float64Row(z, t, k, p)
                kept = model.kept_set(SC.EPS)
                assert kept
                for d in range(SC.GENERAL_DRAWS):
                    u = SR.u24_of(seed, d) / 2.0 ** 24
                    tokens = set().union(*(model.token_set(n, u, SC.EPS) for n in kept))
                    assert tokens
                    ambiguous += len(kept) > 1 or len(tokens) > 1
            assert ambiguous <= 0.05 * SC.GENERAL_BATCH * SC.GENERAL_DRAWS, (vocab, t, k, p, ambiguous)


def test_philox_draws_are_24_bits_and_differ_by_counter():
    draws = [SR.u24_of(1, d) for d in range(64)]
    assert all(0 <= u < 1 << 24 for u in draws) and len(set(draws)) == 64
    assert SR.u24_of(1 << 32, 0) != SR.u24_of(0, 0) and SR.u24_of(0, 1 << 32) != SR.u24_of(0, 0)        # the high words count


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_exports():
    import os
    import re
    from np_modeling_amd import _C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'npm_hip.h')).read()
    body = re.search(r'typedef struct npm_sample \{(.*?)\} npm_sample;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n.strip().lstrip('*') for decl in body.split(';') if decl.strip()
             for n in re.sub(r'^\s*(const\s+)?(float|int32_t|int64_t|uint64_t)\s*\*?', '', decl.strip()).split(',')]
    assert names == [f[0] for f in _C.npm_sample._fields_]
    assert int(re.search(r'#define NPM_SAMPLE_LDS_ROW (\d+)', text).group(1)) == _C.SAMPLE_LDS_ROW
    if os.path.exists(_C.LIB_PATH):
        lib = ctypes.CDLL(_C.LIB_PATH)
        for name in ('npm_sample_rows', 'npm_last_sample_kernel', 'npm_take_rows', 'npm_embedding_bwd'):
            assert hasattr(lib, name)
