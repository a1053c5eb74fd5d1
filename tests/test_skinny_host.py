"""CPU: the dispatch of the skinny-M GEMM without a GPU, on the simulator of tests/hostsim/ (profile 'skinny').

* a decode step with B T <= ``device.SKINNY_MAX_M`` rows records exactly the six (unpacked: eight) ``npm_sgemm_skinny`` calls of
  tests/skinny_cases.py ``decode_products`` and no ``npm_sgemm``; above the threshold it records ``npm_sgemm`` only;
* ``forward`` / ``backward`` at tiny M, ``start_decoding`` (``fill_cache``) and ``admit`` never record a skinny call;
* ``SKINNY_GEMM`` off, a math mode other than f32, a library handle without the entry points and an unsupported shape fall back;
* outputs are array_equal between the two routes; contiguous, ragged and paged caches take the same dispatch;
* header, ``_C.py`` and ``NPM_SKINNY_MAX_M`` agree.

Every test names ``npm_sgemm_skinny`` or ``SKINNY_GEMM``: none exists without this feature.
"""

import ctypes
import os
import re

import numpy as np
import pytest

import decode_cases as DC
import hostsim
from hostsim.fixtures import built, npm_fixture
import skinny_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


npm = npm_fixture('skinny')


def _gemms(calls):
    return [c for c in calls if c.startswith('npm_sgemm')]


def _decode_run(npm, dec, q, kv, sizes, capacity=32, **cache):
    """Outputs of ``dec.decode`` over the chunks of ``q`` and the simulator calls of the decode steps alone."""
    state = dec.start_decoding(kv, capacity, **cache)
    first = len(npm.sim.calls)
    outs = [np.asarray(dec.decode(np.ascontiguousarray(piece), state)) for piece in DC.split(q, sizes)]
    return outs, npm.sim.calls[first:]


@pytest.mark.parametrize('packed', [True, False])
@pytest.mark.parametrize('norm_first', [True, False])
def test_a_decode_step_records_exactly_its_skinny_products(npm, monkeypatch, packed, norm_first):
    D = npm.device
    monkeypatch.setattr(D, 'PACK_QKV', packed)
    f, hidden, heads, kv_heads, batch = 64, 96, 4, 2, 3
    dec, _ = DC.make_decoder(npm, f, heads, kv_heads, hidden, norm_first, True, seed=3, batch=batch)
    rng = np.random.default_rng(0)
    q, kv = rng.standard_normal([batch, 6, f]).astype(np.float32), rng.standard_normal([batch, 7, f]).astype(np.float32)
    assert D.SKINNY_GEMM and 16 <= D.SKINNY_MAX_M <= 64
    for tokens in (5, 1):
        before = len(npm.sim.skinny)
        _, calls = _decode_run(npm, dec, q[:, :tokens], kv, [tokens])
        assert _gemms(calls) == ['npm_sgemm_skinny'] * (6 if packed else 8)
        assert npm.sim.skinny[before:] == SC.decode_products(f, hidden, heads, kv_heads, batch * tokens, packed)
    assert npm.sim.npm_last_skinny_kernel().decode().startswith('sgemm_skinny_kernel NN M=3 N=64 K=96 ')
    assert npm._C.last_skinny_kernel() == npm.sim.last_skinny


def test_above_the_threshold_a_decode_step_is_npm_sgemm_only(npm, monkeypatch):
    D = npm.device
    f = 64
    dec, _ = DC.make_decoder(npm, f, 4, 2, 96, True, True, seed=4, batch=5)
    rng = np.random.default_rng(1)
    q, kv = rng.standard_normal([5, 13, f]).astype(np.float32), rng.standard_normal([5, 7, f]).astype(np.float32)
    assert 5 * 13 > 64 >= D.SKINNY_MAX_M
    _, calls = _decode_run(npm, dec, q, kv, [13])
    assert _gemms(calls).count('npm_sgemm') >= 6 and 'npm_sgemm_skinny' not in calls
    monkeypatch.setattr(D, 'SKINNY_MAX_M', 9)                            # the threshold is what decides: 2 x 5 rows are above 9, 5 are not
    _, calls = _decode_run(npm, dec, q[:2, :5], kv[:2], [5])
    assert 'npm_sgemm_skinny' not in calls
    _, calls = _decode_run(npm, dec, q[:1, :5], kv[:1], [5])
    assert _gemms(calls) == ['npm_sgemm_skinny'] * 6


def test_training_prefill_and_admit_keep_the_training_gemm(npm):
    f = 64
    dec, _ = DC.make_decoder(npm, f, 4, 2, 96, True, True, seed=5, batch=2)
    rng = np.random.default_rng(2)
    q, kv = rng.standard_normal([2, 3, f]).astype(np.float32), rng.standard_normal([2, 7, f]).astype(np.float32)
    first = len(npm.sim.calls)
    y = dec(q, kv)                                                        # forward at M = 6
    dec.backward(np.ones_like(np.asarray(y)), DC.GradRecorder())
    att, _ = DC.make_mha(npm, f, 4, 2, seed=6)
    att.backward(np.ones([2, 2, f], dtype=np.float32), DC.GradRecorder())
    npm.layers.Dense(32)(q.reshape(6, f))
    state = dec.start_decoding(kv, 16, page_size=16, pages=4)             # fill_cache: M = 14 rows of memory
    state.release(1)
    dec.admit(state, 1, kv[:1, :4])                                       # M = 4
    calls = npm.sim.calls[first:]
    assert calls.count('npm_sgemm') > 20 and 'npm_sgemm_skinny' not in calls and npm.sim.skinny == []
    dec.decode(q[:, :1], state)
    assert len(npm.sim.skinny) == 6                                       # ... and the decode step behind them does not


def test_switch_math_mode_old_handle_and_shape_fall_back_with_equal_outputs(npm, monkeypatch):
    D = npm.device
    f = 64
    dec, _ = DC.make_decoder(npm, f, 4, 2, 96, False, True, seed=7, batch=2)
    rng = np.random.default_rng(3)
    q, kv = rng.standard_normal([2, 6, f]).astype(np.float32), rng.standard_normal([2, 7, f]).astype(np.float32)
    want, calls = _decode_run(npm, dec, q, kv, [4, 1, 1])
    assert _gemms(calls) == ['npm_sgemm_skinny'] * 18

    def fallen_back():
        got, calls = _decode_run(npm, dec, q, kv, [4, 1, 1])
        assert _gemms(calls) == ['npm_sgemm'] * 18
        for a, b in zip(got, want):
            assert np.array_equal(a, b)

    with monkeypatch.context() as m:
        m.setattr(D, 'SKINNY_GEMM', False)
        fallen_back()
    npm.set_math('bf16x3')
    fallen_back()
    npm.set_math('f32')
    old = hostsim.install('paged')                                        # a handle of the earlier ABI: no entry points
    assert not hasattr(old, 'npm_sgemm_skinny')
    npm.sim = old
    fallen_back()
    npm.sim = hostsim.install('skinny')
    got, calls = _decode_run(npm, dec, q, kv, [4, 1, 1])
    assert _gemms(calls) == ['npm_sgemm_skinny'] * 18 and all(np.array_equal(a, b) for a, b in zip(got, want))

    # a feature size that is not a multiple of 16: npm_sgemm_skinny_supported says no for every product, nothing is attempted
    att40, _ = DC.make_mha(npm, 40, 2, 2, seed=8)                        # head size 20: the GEMM composition, K = 40
    cache = att40.make_cache(2, 8)
    first = len(npm.sim.calls)
    for piece in (rng.standard_normal([2, 3, 40]).astype(np.float32), rng.standard_normal([2, 1, 40]).astype(np.float32)):
        att40(piece, cache=cache)
    calls = npm.sim.calls[first:]
    assert 'npm_sgemm_skinny' not in calls and calls.count('npm_sgemm') >= 4 and att40._cached_path == 'gemm'
    g = npm._C.npm_gemm()
    assert npm.sim.npm_sgemm_skinny(ctypes.byref(g)) == 10003             # the entry point itself refuses what it does not take


@pytest.mark.parametrize('heads,kv_heads', [(4, 4), (8, 2)])
def test_contiguous_ragged_and_paged_caches_take_the_same_dispatch(npm, monkeypatch, heads, kv_heads):
    D = npm.device
    f = 128
    att, _ = DC.make_mha(npm, f, heads, kv_heads, seed=9, batch=3)
    rng = np.random.default_rng(4)
    x = rng.standard_normal([3, 4, f]).astype(np.float32)
    step = rng.standard_normal([3, 1, f]).astype(np.float32)
    runs = {}
    for on in (True, False):
        monkeypatch.setattr(D, 'SKINNY_GEMM', on)
        for kind, kwargs, lengths in (('contiguous', {}, None), ('ragged', {}, [4, 2, 3]), ('paged', dict(page_size=16), [4, 2, 3])):
            cache = att.make_cache(3, 16, **kwargs)
            first = len(npm.sim.calls)
            outs = [np.asarray(att(x, cache=cache, new_lengths=lengths)), np.asarray(att(step, cache=cache))]
            calls = npm.sim.calls[first:]
            want = 'npm_sgemm_skinny' if on else 'npm_sgemm'
            assert [c for c in _gemms(calls)] == [want] * 4, (kind, on, calls)    # packed q/k/v and the output projection, twice
            runs[kind, on] = outs
    for kind in ('contiguous', 'ragged', 'paged'):
        for a, b in zip(runs[kind, True], runs[kind, False]):
            assert np.array_equal(a, b)
    for a, b in zip(runs['ragged', True], runs['paged', True]):
        assert np.array_equal(a, b)


def test_dense1_drops_the_saved_pre_activation_only_on_the_skinny_route(npm, monkeypatch):
    D = npm.device
    dec, _ = DC.make_decoder(npm, 64, 4, 2, 96, True, True, seed=10, batch=2)
    rng = np.random.default_rng(5)
    q, kv = rng.standard_normal([2, 1, 64]).astype(np.float32), rng.standard_normal([2, 7, 64]).astype(np.float32)
    _decode_run(npm, dec, q, kv, [1])
    assert npm.sim.skinny[-2] == ('NN', 2, 96, 64, SC.EPI_BIAS | SC.EPI_RELU)
    seen = []
    real = npm.sim.npm_sgemm
    monkeypatch.setattr(npm.sim, 'npm_sgemm', lambda gref: (seen.append(gref._obj.epilogue), real(gref))[1])
    monkeypatch.setattr(D, 'SKINNY_GEMM', False)
    _decode_run(npm, dec, q, kv, [1])
    assert seen[-2] == SC.EPI_BIAS | SC.EPI_RELU_SAVE                     # the fallback is the call it always was


def test_the_simulator_restates_the_split_rule_and_the_support_rule(npm):
    sim = npm.sim
    assert [sim.npm_sgemm_skinny_splits(n, k, 1) for n, k in SC.SHAPES] == [1, 1, 4, 8, 8, 8, 8, 16]
    buf = npm.device.empty([64 * 80])
    g = npm._C.npm_gemm()
    g.trans_b, g.m, g.n, g.k, g.batch0, g.batch1 = 1, 8, 32, 48, 1, 1
    g.a, g.lda, g.b, g.ldb, g.c, g.ldc = buf.ptr, 48, buf.ptr, 48, buf.ptr, 32
    assert sim.npm_sgemm_skinny_supported(ctypes.byref(g)) == 1
    for field, value in (('trans_a', 1), ('batch1', 2), ('m', 65), ('m', 0), ('n', 40), ('k', 8), ('lda', 44), ('ldc', 30), ('epilogue', 8),
                         ('epilogue', 1), ('epilogue', 20), ('bsum', buf.ptr), ('colsum', buf.ptr), ('split_k', 2), ('a', buf.ptr + 4)):
        saved = getattr(g, field)
        setattr(g, field, value)
        assert sim.npm_sgemm_skinny_supported(ctypes.byref(g)) == 0, field
        setattr(g, field, saved)
    assert sim.npm_sgemm_skinny_supported(ctypes.byref(g)) == 1


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_skinny_entry_points_header_against_bindings(built):
    _C = built
    text = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    assert int(re.search(r'#define\s+NPM_SKINNY_MAX_M\s+(\d+)', text).group(1)) == _C.SKINNY_MAX_M == hostsim.gemm.MAX_M == 64
    assert int(re.search(r'#define\s+NPM_SKINNY_MAX_SPLITS\s+(\d+)', text).group(1)) == _C.SKINNY_MAX_SPLITS == hostsim.gemm.MAX_SPLITS
    assert int(re.search(r'NPM_TUNE_SKINNY_SPLITS\s*=\s*(\d+)', text).group(1)) == _C.TUNE_SKINNY_SPLITS == 22
    assert int(re.search(r'NPM_TUNE_SKINNY_NT\s*=\s*(\d+)', text).group(1)) == _C.TUNE_SKINNY_NT == 23
    assert int(re.search(r'#define\s+NPM_ABI_VERSION\s+(\d+)', text).group(1)) == 2
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    gemm = ctypes.POINTER(_C.npm_gemm)
    for name, decl, want in (('npm_sgemm_skinny', r'int npm_sgemm_skinny\(const npm_gemm \*g\);', [gemm]),
                             ('npm_sgemm_skinny_supported', r'int npm_sgemm_skinny_supported\(const npm_gemm \*g\);', [gemm]),
                             ('npm_sgemm_skinny_splits', r'int npm_sgemm_skinny_splits\(int n, int k, int trans_b\);', [ctypes.c_int] * 3)):
        assert re.search(decl, code), name
        assert _C.SIGNATURES[name] == want
    assert re.search(r'const char \*npm_last_skinny_kernel\(void\);', code) and _C._SPECIAL['npm_last_skinny_kernel'] == (ctypes.c_char_p, [])
    from np_modeling_amd import device as D
    assert D.SKINNY_MAX_M <= _C.SKINNY_MAX_M
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name in ('npm_sgemm_skinny', 'npm_sgemm_skinny_supported', 'npm_sgemm_skinny_splits', 'npm_last_skinny_kernel'):
        assert hasattr(lib, name), f'{name} not exported'
    bound = _C.load_library()
    assert bound.npm_abi_version() == 2 and bound.npm_last_skinny_kernel() == b''
    assert [bound.npm_sgemm_skinny_splits(n, k, t) for n, k in SC.SHAPES for t in (0, 1)] == \
        [hostsim.gemm.auto_splits(n, k) for n, k in SC.SHAPES for _ in (0, 1)]
    assert bound.npm_sgemm_skinny_supported(None) == 0 and bound.npm_sgemm_skinny_supported(ctypes.byref(_C.npm_gemm())) == 0
    count = ctypes.c_int(-1)
    bound.npm_device_count(ctypes.byref(count))
    if count.value == 0:                                                  # no compute without a GPU, as every entry point
        assert bound.npm_sgemm_skinny(ctypes.byref(_C.npm_gemm())) == 10001
