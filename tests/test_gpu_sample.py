"""GPU: npm_sample_rows (csrc/npm_sample.hip) through the C ABI against tests/sample_reference.py, on the case lists of
tests/sample_cases.py (whose properties tests/test_sample_host.py checks on the reference alone).

Bounds.  (a) exact rows -- logits from {c, -200, -inf}, so every weight is 2^32 or 0 whatever the exponential's last bit: token,
kept, prob and the advanced counter must EQUAL the integer model.  (d) general rows against float64: the kernel's answer must be
admissible within eps = 2e-5 of the row's mass.  A weight's relative error is at most two fp32 roundings of an exponent argument
no larger than 88 in magnitude, 2 * 88 * 2^-24 = 1.05e-5, plus the exponential's own few ulps and the floor's V * 2^-32; integer
sums add nothing; 2e-5 is under twice that.  With the reference's cumulative masses c in order, kept = n needs c_n >= (p - eps) R1
(or n = |K1|) and c_{n-1} < (p + eps) R1; the token i must lie in the first n tokens in order with s_{i-1} <= (u + eps) Rk and
s_i > (u - eps) Rk for the running mass s in index order -- so every pair that admits one answer gets exactly it.  prob: 1e-4
relative (twice eps for the quotient of two masses, and the fp32 rounding).  (b), (c), (e): equalities.

Every test here needs ``npm_sample_rows``: none passes on the parent commit.
"""

import numpy as np
import pytest

import sample_cases as SC
import sample_reference as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


def _last_kernel():
    from np_modeling_amd import _C
    return _C.last_sample_kernel()


# ---- (a) exact rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vocab', SC.EXACT_VOCABS)
def test_exact_rows_equal_the_integer_model(npm, vocab):
    rows = SC.exact_rows(vocab)
    orders = [SR.order_of(z) for z in rows]
    weights = {t: [SR.exact_weights(z, t) for z in rows] for t in (0.5, 1.0, 3.0)}
    call = SC.Call(npm, rows, 1.0, 0, 1.0, SC.EXACT_SEEDS)
    for t, k, p in SC.exact_params(vocab):
        call.set_params(t, k, p, SC.EXACT_SEEDS)
        models = [SR.ExactRow(z, t, k, p, w=weights[t][r] if t else None, order=o) for r, (z, o) in enumerate(zip(rows, orders))]
        for d in range(SC.EXACT_DRAWS):
            token, kept, prob, draw = call.step()
            want = [m.draw(seed, d) for m, seed in zip(models, SC.EXACT_SEEDS)]
            assert token.tolist() == [w[0] for w in want], (vocab, t, k, p, d)
            assert kept.tolist() == [w[1] for w in want], (vocab, t, k, p, d)
            assert np.array_equal(SC.bits(prob), SC.bits([w[2] for w in want])), (vocab, t, k, p, d)
            assert draw.tolist() == [d + 1] * 4
    assert ('row=lds' if vocab <= SC.LDS_ROW else 'row=global') in _last_kernel() and f'V={vocab}' in _last_kernel()


# ---- (b) layout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vocab', [1000, SC.LDS_ROW + 1])
def test_pitch_padding_and_a_misaligned_base_change_nothing(npm, vocab):
    """Pitch V + 5 with +inf / NaN in the padding columns (they neither win nor invalidate the row), and a base 4 bytes off
    16-byte alignment: the tokens of the aligned, dense call.  The guard words around token / kept / prob / draw are checked
    by every step."""
    rows = np.concatenate([SC.general_rows(8195)[:2, :vocab] if vocab <= 8195 else
                           (4 * np.random.default_rng(7).standard_normal([2, vocab])).astype(np.float32), SC.exact_rows(vocab)[:2]])
    params = dict(temperature=[0.7, 0.0, 1.0, 3.0], top_k=[50, 0, 5, 0], top_p=[0.9, 1.0, 1.0, 0.25], seed=[3, 4, 5, 6])
    results = {}
    for name, layout in dict(dense={}, pitched=dict(pitch=vocab + 5), shifted=dict(offset=1), pitch8=dict(pitch=vocab + 8 - vocab % 4)).items():
        call = SC.Call(npm, rows, **params, **layout)
        results[name] = [call.step() for _ in range(8)]
        vec = name in ('dense', 'pitch8') and vocab % 4 == 0 or name == 'pitch8'
        assert ('vec' if vec else 'scalar') in _last_kernel(), (name, _last_kernel())
    for name in ('pitched', 'shifted', 'pitch8'):
        for got, want in zip(results[name], results['dense']):
            assert all(np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)
                       for g, w in zip(got, want)), name
    assert all((step[0] >= 0).all() and (step[0] < vocab).all() for step in results['dense'])


# ---- (c) invalid and inactive rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('what', ['nan', 'inf', 'all-masked'])
@pytest.mark.parametrize('vocab', [255, SC.LDS_ROW + 1])
def test_an_invalid_row_gives_minus_one_beside_untouched_neighbours(npm, what, vocab):
    rows = (4 * np.random.default_rng(8).standard_normal([3, vocab])).astype(np.float32)
    params = dict(temperature=0.9, top_k=[0, 20, 7], top_p=[0.8, 0.9, 1.0], seed=[1, 2, 3])
    clean = SC.Call(npm, rows, **params).step()
    broken = rows.copy()
    if what == 'all-masked':
        broken[1] = -np.inf
    else:
        broken[1, vocab - 1] = np.nan if what == 'nan' else np.inf
    token, kept, prob, draw = SC.Call(npm, broken, **params).step()
    assert (token[1], kept[1], prob[1]) == (-1, 0, 0) and draw.tolist() == [1, 1, 1]
    for b in (0, 2):
        assert (token[b], kept[b], SC.bits(prob)[b]) == (clean[0][b], clean[1][b], SC.bits(clean[2])[b])


def test_an_inactive_row_is_left_alone_and_not_read(npm):
    rows = (4 * np.random.default_rng(9).standard_normal([3, 1000])).astype(np.float32)
    params = dict(temperature=0.9, top_k=[0, 20, 7], top_p=[0.8, 0.9, 1.0], seed=[1, 2, 3])
    clean = SC.Call(npm, rows, **params, draw=[5, 6, 7]).step()
    for poison in (False, True):
        x = rows.copy()
        if poison:
            x[1] = np.nan
        token, kept, prob, draw = SC.Call(npm, x, **params, draw=[5, 6, 7], active=[1, 0, 1]).step()
        assert (token[1], kept[1], prob[1]) == (-1, 0, 0)
        assert draw.tolist() == [6, 6, 8]                                  # row 1's counter did not move
        for b in (0, 2):
            assert (token[b], kept[b], SC.bits(prob)[b]) == (clean[0][b], clean[1][b], SC.bits(clean[2])[b])
    assert clean[3].tolist() == [6, 7, 8]


def test_bad_arguments_are_refused_before_a_launch(npm):
    import ctypes
    from np_modeling_amd import _C
    call = SC.Call(npm, np.zeros([2, 8], dtype=np.float32), 1.0, 0, 1.0, 0)
    p = call.params.ptr
    good = dict(logits=call.logits.ptr, pitch=8, batch=2, vocab=8, temperature=p + 16, top_k=p + 24, top_p=p + 32, seed=p,
                draw=call.draws.ptr + 8 * SC.GUARD, token=call.out.ptr)
    assert _C.lib().npm_sample_rows(ctypes.byref(_C.npm_sample(**good))) == 0
    for change in (dict(pitch=7), dict(batch=0), dict(vocab=0), dict(vocab=(1 << 20) + 1, pitch=1 << 21), dict(logits=None),
                   dict(temperature=None), dict(top_k=None), dict(top_p=None), dict(seed=None), dict(draw=None), dict(token=None)):
        assert _C.lib().npm_sample_rows(ctypes.byref(_C.npm_sample(**{**good, **change}))) == 10002, change
        assert b'npm_sample_rows' in _C.lib().npm_last_error()
    assert _C.lib().npm_sample_rows(None) == 10002


# ---- (d) general rows against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vocab', SC.GENERAL_VOCABS)
def test_general_rows_are_admissible_against_float64(npm, vocab):
    rows = SC.general_rows(vocab)
    call = SC.Call(npm, rows, 1.0, 0, 1.0, SC.GENERAL_SEEDS)
    for t, k, p in SC.GENERAL_FAMILIES:
        call.set_params(t, k, p, SC.GENERAL_SEEDS)
        models = [SR.Float64Row(z, t, k, p) for z in rows]
        kept_sets = [m.kept_set(SC.EPS) for m in models]
        for d in range(SC.GENERAL_DRAWS):
            token, kept, prob, draw = call.step()
            assert draw.tolist() == [d + 1] * SC.GENERAL_BATCH
            for b, (model, seed) in enumerate(zip(models, SC.GENERAL_SEEDS)):
                where = (vocab, t, k, p, d, b)
                assert kept[b] in kept_sets[b], (where, int(kept[b]), kept_sets[b])
                allowed = model.token_set(int(kept[b]), SR.u24_of(seed, d) / 2.0 ** 24, SC.EPS)
                assert token[b] in allowed, (where, int(token[b]), allowed)
                want = model.prob(int(kept[b]), int(token[b]))
                assert abs(float(prob[b]) - want) <= 1e-4 * want, (where, float(prob[b]), want)


# ---- (e) independence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vocab', [8195, SC.LDS_ROW + 1])
def test_a_row_does_not_depend_on_its_batch_and_launches_repeat_bitwise(npm, vocab):
    rows = (4 * np.random.default_rng(10).standard_normal([4, vocab])).astype(np.float32)
    params = dict(temperature=[0.7, 1.3, 0.7, 1.0], top_k=[0, 50, 50, 0], top_p=[0.9, 1.0, 0.9, 1.0])
    seeds, start = [21, 22, 23, 24], [0, 3, 1 << 33, 7]
    as_bits = lambda step: [a.view(np.uint32) if a.dtype == np.float32 else a for a in step]
    batch = as_bits(SC.Call(npm, rows, **params, seed=seeds, draw=start).step())
    again = as_bits(SC.Call(npm, rows, **params, seed=seeds, draw=start).step())
    assert all(np.array_equal(a, b) for a, b in zip(batch, again))
    for b in range(4):
        alone = as_bits(SC.Call(npm, rows[b:b + 1], **{k: [v[b]] for k, v in params.items()}, seed=[seeds[b]], draw=[start[b]]).step())
        assert all(np.array_equal(a[0], x[b]) for a, x in zip(alone, batch)), b


def test_counters_0_to_63_in_one_batch_give_what_64_successive_calls_give(npm):
    z = (4 * np.random.default_rng(11).standard_normal([1, 1000])).astype(np.float32)
    params = dict(temperature=1.3, top_k=50, top_p=0.95, seed=31)
    one = SC.Call(npm, z, **params)
    successive = [one.step() for _ in range(64)]
    assert [int(s[3][0]) for s in successive] == list(range(1, 65))
    token, kept, prob, draw = SC.Call(npm, np.repeat(z, 64, axis=0), **params, draw=np.arange(64)).step()      # B 64: the one wide batch here
    assert token.tolist() == [int(s[0][0]) for s in successive] and kept.tolist() == [int(s[1][0]) for s in successive]
    assert np.array_equal(SC.bits(prob), SC.bits([s[2][0] for s in successive])) and draw.tolist() == list(range(1, 65))
    assert len(set(token.tolist())) > 4                                      # the draws do differ
