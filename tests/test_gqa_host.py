"""CPU: grouped-query attention's C ABI is exported and bound, and the float64 restatement the GPU tests compare against
(tests/gqa_reference.py: the reference's gqa_fwd, layers/attentions_test.py:282-333, plus a hand-derived backward) is right:
against central finite differences, against the oracle's MHA when Hkv == Hq, and against MHA with repeated K / V weights."""

import ctypes
import os
import re

import numpy as np
import pytest

import gqa_reference as G
from oracle import np_oracle as O
from hostsim.fixtures import built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPED = ('npm_mha_core_fwd_grouped', 'npm_mha_core_bwd_grouped')


def test_grouped_entry_points_are_declared_exported_and_bound(built):
    _C = built
    with open(os.path.join(ROOT, 'include', 'npm_hip.h')) as f:
        header = f.read()
    for name in GROUPED:
        assert re.search(r'\bint\s+%s\s*\(\s*const npm_mha_core \*c,\s*int32_t kv_heads\s*\)' % name, header), name
        assert _C.SIGNATURES[name] == [ctypes.POINTER(_C.npm_mha_core), ctypes.c_int32]
        assert hasattr(ctypes.CDLL(_C.LIB_PATH), name), f'{name} not exported'
    lib = _C.load_library()
    for name in GROUPED:
        fn = getattr(lib, name)
        assert fn.argtypes == [ctypes.POINTER(_C.npm_mha_core), ctypes.c_int32] and fn.restype is ctypes.c_int


def _problem(seed, b, sq, skv, f, hq, hkv, cross=False):
    rng = np.random.default_rng(seed)
    p = G.init_params(rng, f, f, hq, hkv, scale=0.5)
    query = rng.standard_normal([b, sq, f])
    key = rng.standard_normal([b, skv, f]) if cross else query
    value = rng.standard_normal([b, skv, f]) if cross else query
    dy = rng.standard_normal([b, sq, f])
    return rng, p, query, key, value, dy


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('hq,hkv', [(4, 2), (4, 1), (6, 3)])
def test_restatement_backward_matches_finite_differences(hq, hkv, masked):
    f = 2 * hq
    rng, p, query, key, value, dy = _problem(hq * 10 + hkv, 2, 3, 4, f, hq, hkv, cross=True)
    mask = None
    if masked:
        mask = rng.random([2, hq, 3, 4]) < 0.6
        mask[..., 0] = True

    def loss(p_, q_, k_, v_):
        return float(np.sum(G.gqa_fwd(p_, q_, k_, v_, mask)[0] * dy))

    _, cache = G.gqa_fwd(p, query, key, value, mask)
    (dq, dk, dv), grads = G.gqa_bwd(p, cache, dy)
    eps = 1e-6

    def numeric(arr, bump):
        out = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            saved = arr[i]
            arr[i] = saved + eps
            up = bump()
            arr[i] = saved - eps
            down = bump()
            arr[i] = saved
            out[i] = (up - down) / (2 * eps)
        return out

    for name in p:
        np.testing.assert_allclose(grads[name], numeric(p[name], lambda: loss(p, query, key, value)), rtol=1e-6, atol=1e-6,
                                   err_msg=name)
    for name, arr, want in (('query', query, dq), ('key', key, dk), ('value', value, dv)):
        np.testing.assert_allclose(want, numeric(arr, lambda: loss(p, query, key, value)), rtol=1e-6, atol=1e-6, err_msg=name)


@pytest.mark.parametrize('cross', [False, True])
def test_restatement_with_as_many_kv_heads_as_query_heads_is_the_oracle_mha(cross):
    _, p, query, key, value, dy = _problem(3, 2, 5, 7 if cross else 5, 16, 4, 4, cross=cross)
    out, cache = G.gqa_fwd(p, query, key, value)
    want, wcache = O.mha_fwd(p, query, key, value)
    np.testing.assert_allclose(out, want, rtol=1e-12, atol=1e-12)
    got_in, got = G.gqa_bwd(p, cache, dy)
    want_in, wg = O.mha_bwd(p, wcache, dy)
    for a, b_ in zip(got_in, want_in):
        np.testing.assert_allclose(a, b_, rtol=1e-12, atol=1e-12)
    for name in p:
        np.testing.assert_allclose(got[name], wg[name], rtol=1e-12, atol=1e-12, err_msg=name)


@pytest.mark.parametrize('hq,hkv', [(8, 4), (8, 2), (8, 1), (6, 2)])
def test_gqa_is_mha_with_repeated_kv_weights(hq, hkv):
    """GQA == MHA whose K / V weights repeat with period Hkv (wk_full[h] = wk[h % Hkv]); dwk / dbk / dwv / dbv are the group
    sums of MHA's.  This pins the head mapping h -> h % Hkv (the np.repeat of the reference's Flax setup, h -> h // G,
    would fail it)."""
    _, p, query, key, value, dy = _problem(hq + hkv, 2, 6, 9, 2 * hq, hq, hkv, cross=True)
    full = dict(p)
    idx = np.arange(hq) % hkv
    for n in ('wk', 'wv', 'bk', 'bv'):
        full[n] = p[n][idx]
    out, cache = G.gqa_fwd(p, query, key, value)
    want, wcache = O.mha_fwd(full, query, key, value)
    np.testing.assert_allclose(out, want, rtol=1e-12, atol=1e-12)
    got_in, got = G.gqa_bwd(p, cache, dy)
    want_in, wg = O.mha_bwd(full, wcache, dy)
    for a, b_ in zip(got_in, want_in):
        np.testing.assert_allclose(a, b_, rtol=1e-11, atol=1e-11)
    for n in ('wq', 'wo', 'bq', 'bo'):
        np.testing.assert_allclose(got[n], wg[n], rtol=1e-11, atol=1e-11, err_msg=n)
    for n in ('wk', 'wv', 'bk', 'bv'):
        sums = wg[n].reshape((hq // hkv, hkv) + wg[n].shape[1:]).sum(axis=0)       # head h = g * Hkv + c summed over g
        np.testing.assert_allclose(got[n], sums, rtol=1e-11, atol=1e-11, err_msg=n)
    if hkv > 1 and hq // hkv > 1:                  # the other convention (h -> h // G) is a different function
        other = dict(full)
        for n in ('wk', 'wv', 'bk', 'bv'):
            other[n] = np.repeat(p[n], hq // hkv, axis=0)
        assert np.abs(O.mha_fwd(other, query, key, value)[0] - out).max() > 1e-6
