"""CPU: the constructions of tests/attn_range_data.py do what tests/test_gpu_attn_range.py relies on -- the lazy reference
point of the fused forward kernels moves after the first tile, rows that did not trigger rescale by an alpha strictly
inside (0, 1), probabilities near 2^10 accumulate, masks hide the largest scores -- and its float64 reference and bound
agree with the oracle and admit a float32 evaluation."""

import numpy as np
import pytest

import attn_range_data as R
from oracle import np_oracle as O

SQ, SKV = 100, 300                     # the shapes of group A (test_gpu_attn_range.py LAZY_SHAPE)


@pytest.fixture(scope='module')
def lazy():
    return {masked: R.lazy_problem(2, 4, 2, SQ, SKV, 64, 11, masked) for masked in (False, True)}


def _stats(data, bi, hi, wave, masked):
    q, k, _, _, scale, mask = data
    s2 = R.plane_scores_log2(q, k, scale, bi, hi, mask if masked else None)
    return s2, R.simulate_lazy(s2, wave)


@pytest.mark.parametrize('wave', R.WAVES)
def test_scores_are_exact_and_bounded(lazy, wave):
    q, k, _, _, scale, _ = lazy[False]
    raw = q[0, :, 0].astype(np.float64) @ k[0, :, 0].astype(np.float64).T
    assert np.array_equal(raw, np.round(raw)) and np.abs(raw).max() < 2 ** 24      # integers: exact in float32 products and sums
    assert np.all(np.abs(q) < 2 ** 11) and np.all(q == np.round(q)) and np.all(k == np.round(k))
    for bi in range(2):
        for hi in range(4):
            s2, _ = _stats(lazy[False], bi, hi, wave, False)
            assert np.abs(s2).max() / R.LOG2E <= 48                                  # |scaled score| about 40 at most
            # no tile maximum within 1e-3 log2 units of a threshold crossing (float32 rounds tmax c by ~1e-5): the kernels branch as modelled
            nt = (SKV + 31) // 32
            tmax = np.stack([s2[:, 32 * t:32 * t + 32].max(axis=1) for t in range(nt)], axis=1)
            gaps = (tmax[:, :, None] - tmax[:, None, :] - R.RESCALE).ravel()
            assert np.abs(gaps).min() > 1e-3


@pytest.mark.parametrize('wave', R.WAVES)
def test_climb_moves_on_every_tile_and_rescales_rows_that_did_not_trigger(lazy, wave):
    nt = (SKV + 31) // 32
    for bi in range(2):
        s2, st = _stats(lazy[False], bi, 0, wave, False)
        climbers = ((np.arange(SQ) + 3 * bi) % 5) == 0
        assert (st['moves'][climbers] == nt - 1).all()                               # a move on every tile after the first
        alphas = np.array([a for r, t, a in st['alpha']])
        assert len(alphas) >= 100 and (alphas > 2 ** -12).all() and (alphas < 1).all()
        assert (alphas < 0.2).sum() >= 20 and (alphas > 0.5).sum() >= 20             # small and large alphas both
        rows = {r // wave for r, t, a in st['alpha']}
        assert rows == set(range((SQ + wave - 1) // wave))                          # in every wave


@pytest.mark.parametrize('wave', R.WAVES)
def test_just_under_the_threshold_moves_every_other_tile(lazy, wave):
    nt = (SKV + 31) // 32
    for bi in range(2):
        s2, st = _stats(lazy[False], bi, 1, wave, False)
        under = np.arange(SQ) % 3 < 2
        assert (st['moves'][under] == (nt - 1) // 2).all()
        assert st['peak'][under].min() > 2 ** 9                                      # l accumulates probabilities near 2^10
        assert st['peak'].max() < 2 ** R.RESCALE


@pytest.mark.parametrize('wave', R.WAVES)
def test_edges_put_the_maximum_in_the_ragged_last_or_only_the_first_tile(lazy, wave):
    assert SKV % 32 != 0
    nt = (SKV + 31) // 32
    for bi in range(2):
        s2, st = _stats(lazy[False], bi, 2, wave, False)
        arg = s2.argmax(axis=1) // 32
        j = np.arange(SQ) % 7
        assert (arg[(j == 0) | (j == 3) | (j == 4)] == nt - 1).all()
        assert (arg[(j == 1) | (j == 2) | (j == 6)] == 0).all()
        alphas = np.array([a for r, t, a in st['alpha']])
        assert alphas.min() < 2 ** -9 and alphas.min() > 2 ** -12                   # down to 2^-10 on rows that did not trigger


@pytest.mark.parametrize('wave', R.WAVES)
def test_masked_rows_hide_their_largest_scores(lazy, wave):
    q, k, _, _, scale, mask = lazy[True]
    nt = (SKV + 31) // 32
    for bi in range(2):
        full = R.plane_scores_log2(q, k, scale, bi, 3)
        s2, st = _stats(lazy[True], bi, 3, wave, True)
        assert np.isfinite(s2).any(axis=1).all()                                     # every row keeps a key
        hidden = np.where(mask[bi, 3], -np.inf, full).max(axis=1)
        assert (hidden - s2.max(axis=1) > 5 * R.LOG2E).all()                          # a leak would be out by e^5 at least
        lead = np.arange(SQ) % 4 != 0
        assert (st['first'][lead] >= 1).all()                                         # m = -inf on the first tile(s) ...
        rising = np.arange(SQ) % 4 == 1
        assert (st['moves'][rising] >= nt - 4).all()                                  # ... then finite, then rescaled


@pytest.mark.parametrize('masked', [False, True])
def test_reference_is_the_oracle(masked):
    q, k, v, dctx, scale, mask = R.lazy_problem(1, 4, 4, 40, 120, 16, 3, masked)
    got = R.reference(q, k, v, dctx, scale, mask)
    q64, k64, v64 = (x.astype(np.float64) for x in (q, k, v))
    full = None if mask is None else np.broadcast_to(mask, (1, 4, 40, 120))
    ctx, lse, probs = O.attention_core_fwd(q64, k64, v64, scale, full)
    dq, dk, dv = O.attention_core_bwd(q64, k64, v64, probs, dctx.astype(np.float64), scale)
    for name, want in (('ctx', ctx), ('lse', lse), ('dq', dq), ('dk', dk), ('dv', dv)):
        np.testing.assert_allclose(got[name], want, rtol=1e-12, atol=1e-12, err_msg=name)
    grouped = R.reference(q, k[:, :, :2], v[:, :, :2], dctx, scale, mask)             # head h reads K / V head h % 2
    ctx2, _, probs2 = O.attention_core_fwd(q64, k64[:, :, [0, 1, 0, 1]], v64[:, :, [0, 1, 0, 1]], scale, full)
    np.testing.assert_allclose(grouped['ctx'], ctx2, rtol=1e-12, atol=1e-12)


def test_shift_is_exact_and_moves_lse_by_the_shift():
    q, k, v, dctx, scale, ku, shift = R.shift_problem(1, 4, 2, 48, 70, 64, 5)
    assert 150 < np.abs(shift).max() <= 200.5
    base, moved = R.reference(q, k, v, dctx, scale), R.reference(q, ku, v, dctx, scale)
    np.testing.assert_allclose(moved['lse'] - base['lse'], shift[0][None] if shift.shape[0] == 1 else shift, rtol=0, atol=1e-9)
    for name in ('ctx', 'dq', 'dk', 'dv'):
        np.testing.assert_allclose(moved[name], base[name], rtol=0, atol=1e-9, err_msg=name)


@pytest.mark.parametrize('kind', ['plain', 'shifted', 'saturated'])
def test_bound_reduces_to_the_base_and_admits_float32(kind):
    """X of O(1) data keeps the bound at the existing 2e-6 / 3e-6; in every regime a float32 evaluation of the reference
    formulas stays inside it."""
    rng = np.random.default_rng(7)
    b, h, sq, skv, d = 1, 2, 64, 200, 64
    if kind == 'plain':
        q, k, v, dctx = (rng.standard_normal(s).astype(np.float32) for s in ([b, sq, h, d], [b, skv, h, d], [b, skv, h, d], [b, sq, h, d]))
        scale = 1.0 / np.sqrt(d)
    elif kind == 'shifted':
        q, _, v, dctx, scale, k, _ = R.shift_problem(b, h, h, sq, skv, d, 9)
    else:
        q, k, v, dctx, scale = R.saturated_problem(b, h, h, sq, skv, d, 9)
    want = R.reference(q, k, v, dctx, scale)
    x = R.exponent_magnitude(q, k, scale, want['lse'])
    if kind == 'plain':
        assert R.exponent_tol(2e-6, x) == 2e-6 and R.exponent_tol(3e-6, x) == 3e-6
    f32 = R.float32_reference(q, k, v, dctx, scale)
    for name, base in (('ctx', 2e-6), ('dq', 3e-6), ('dk', 3e-6), ('dv', 3e-6)):
        tol = R.exponent_tol(base, x)
        err = np.abs(f32[name] - want[name]) / (np.abs(want[name]) + np.abs(want[name]).max())
        assert err.max() <= tol, (name, err.max(), tol)
    assert np.abs(f32['lse'] - want['lse']).max() <= R.exponent_tol(3e-6, x)


def test_key_padding_makes_empty_and_half_empty_blocks():
    mask = R.key_padding_mask(R.PAD_LENGTHS, 700)[:, 0, 0]
    vis = mask.reshape(4, -1)
    blocks128 = [np.pad(r, (0, 768 - 700)).reshape(6, 128) for r in vis]
    blocks256 = [np.pad(r, (0, 768 - 700)).reshape(3, 256) for r in vis]
    assert any((~blk.any(axis=1)).any() for blk in blocks128)                      # whole hidden 128-key blocks
    assert any((~blk.any(axis=1)).any() for blk in blocks256)                      # ... and 256-key blocks
    assert any(blk[:, :128].all(axis=1).any() and (~blk[1, 128:]).all() for blk in blocks256[1:2])  # first half visible, second not
    assert any((blk.sum(axis=1) == 1).any() for blk in blocks128)                   # a block with one visible key


def test_gap_mask_sees_only_the_last_tile():
    m = R.gap_mask(2048)[0, 0]
    assert (m[::5, :2016] == 0).all() and m[::5, 2016:].all() and m.any(axis=1).all()
    assert m[2040, 2040] and not m[2041, 2042]
