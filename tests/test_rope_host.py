"""CPU: rotary position embeddings without a GPU, on the simulator of tests/hostsim/ (profile 'rope').

* the reference itself (tests/rope_reference.py): float32 ``rotate`` against float64 with exact angles at the bound the number
  formats give, inverse after forward, and the relative-position property;
* ``rope_base=None`` is the layer without the keyword, call for call;
* where npm_rope is launched: once per forward and once (inverse) per backward on the packed projection, twice each way on
  separate tensors, in front of ``npm_kv_append*`` in a cached forward -- with the ``before`` row of the cache's length mirror for
  ragged and paged calls and no upload more than without rotation;
* errors, the size of the tables, and the layer's results through the simulator against the float64 reference;
* the entry point: header against bindings and exports, the code object of the built kernels.

Every test but the first three needs ``rope_base``, ``npm_rope`` or ``device.RopeTable``, which do not exist without this feature.
"""

import ctypes
import os
import re

import numpy as np
import pytest

import decode_cases as DC
import decode_reference as DR
from hostsim.fixtures import built, npm_fixture
import rope_cases as RC
import rope_reference as RR
from conftest import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 1e4
U = 2.0 ** -24                    # unit roundoff of float32


npm = npm_fixture('rope')


make_mha = RC.make_mha


# ---- the reference itself ---------------------------------------------------------------------------------------------------------
def _reference_data():
    rng = np.random.default_rng(0)
    positions = np.concatenate([np.arange(64), rng.integers(64, 16385, size=192), [16384]])
    x = rng.standard_normal([positions.size, 3, 128]).astype(np.float32)
    return x, positions, RR.tables(16385, 128, BASE)


def test_float32_rotate_is_within_three_roundings_of_float64():
    """One rounding of the table entry, one of each product, one of the sum: |rotate - rotate64| <= 3 u (|x[i]| + |x[i + half]|)
    at positions up to 16384, D 128, N(0, 1) data."""
    x, positions, (cos, sin) = _reference_data()
    pair = np.abs(x[..., :64]) + np.abs(x[..., 64:])
    pair = np.concatenate([pair, pair], axis=-1).astype(np.float64)
    for inverse in (False, True):
        err = np.abs(RR.rotate(x, positions, cos, sin, inverse).astype(np.float64) - RR.rotate64(x, positions, BASE, inverse))
        used = float((err / (U * pair)).max())
        print(f'rotate vs rotate64 (inverse={inverse}): {used:.2f} u (|x[i]| + |x[i + half]|), bound 3')
        assert used <= 3.0


def test_inverse_after_forward_returns_x():
    x, positions, (cos, sin) = _reference_data()
    back = RR.rotate(RR.rotate(x, positions, cos, sin), positions, cos, sin, inverse=True)
    pair = np.abs(x[..., :64]) + np.abs(x[..., 64:])
    pair = np.concatenate([pair, pair], axis=-1).astype(np.float64)
    used = float((np.abs(back.astype(np.float64) - x) / (U * pair)).max())
    print(f'inverse(forward(x)) - x: {used:.2f} u (|x[i]| + |x[i + half]|), bound 6')
    assert used <= 6.0
    exact = RR.rotate64(RR.rotate64(x, positions, BASE), positions, BASE, inverse=True)
    np.testing.assert_allclose(exact, x, rtol=0, atol=1e-13)


def test_rotated_dot_products_depend_on_the_position_difference_only():
    rng = np.random.default_rng(1)
    q, k = rng.standard_normal([1, 1, 2, 32]), rng.standard_normal([1, 1, 2, 32])
    dots = []
    for shift in (0, 5, 1000, 16000):
        qr, kr = RR.rotate64(q, [[7 + shift]], BASE), RR.rotate64(k, [[3 + shift]], BASE)
        dots.append((qr * kr).sum(axis=-1))
    for d in dots[1:]:
        np.testing.assert_allclose(d, dots[0], rtol=0, atol=1e-11)
    other = (RR.rotate64(q, [[8]], BASE) * RR.rotate64(k, [[3]], BASE)).sum(axis=-1)
    assert np.abs(other - dots[0]).max() > 1e-3                           # and on nothing less


def test_a_table_row_does_not_depend_on_the_row_count(npm):
    small, large = RR.tables(8, 12, BASE), RR.tables(4096, 12, BASE)
    assert all(np.array_equal(s, l[:8]) for s, l in zip(small, large))
    product = npm.device.rope_tables(4096, 12, BASE)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(product, large))


# ---- rope_base=None is the layer without the keyword ------------------------------------------------------------------------------
def _schedule(npm, **kwargs):
    """A forward, a backward, a cached prefill, a decode step and a ragged step: (calls, outputs)."""
    att, _ = make_mha(npm, 64, 4, 2, seed=3, **kwargs)
    rng = np.random.default_rng(2)
    x, dy = rng.standard_normal([2, 9, 64]).astype(np.float32), rng.standard_normal([2, 9, 64]).astype(np.float32)
    first = len(npm.sim.calls)
    outs = [np.asarray(att(x))]
    outs += [np.asarray(g) for g in att(dy, backprop=True, optimizer_=DC.GradRecorder())]
    cache = att.make_cache(2, 16)
    outs.append(np.asarray(att(x, cache=cache)))
    outs.append(np.asarray(att(x[:, :1], cache=cache)))
    outs.append(np.asarray(att(x[:, :3], cache=cache, new_lengths=[3, 1])))
    return list(npm.sim.calls[first:]), outs


def test_rope_base_none_makes_the_calls_of_a_layer_without_the_keyword(npm):
    calls_plain, outs_plain = _schedule(npm)
    calls_none, outs_none = _schedule(npm, rope_base=None)
    assert calls_none == calls_plain and 'npm_rope' not in calls_none and len(calls_none) > 10
    for a, b in zip(outs_none, outs_plain):
        assert np.array_equal(a, b)
    calls_rope, outs_rope = _schedule(npm, rope_base=BASE)
    assert calls_rope.count('npm_rope') == 5 and [c for c in calls_rope if c != 'npm_rope'] == calls_plain
    assert np.abs(outs_rope[0] - outs_plain[0]).max() > 1e-3              # the rotation matters


# ---- where npm_rope is launched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('heads,kv_heads', [(4, 4), (4, 2)])
def test_packed_self_attention_rotates_q_and_k_in_one_launch_each_way(npm, heads, kv_heads):
    att, _ = make_mha(npm, 64, heads, kv_heads, seed=4, rope_base=BASE)
    rng = np.random.default_rng(3)
    x = rng.standard_normal([2, 9, 64]).astype(np.float32)
    first, ropes = len(npm.sim.calls), len(npm.sim.ropes)
    att(x)
    calls = npm.sim.calls[first:]
    assert att._packed and calls.count('npm_rope') == 1 and calls.index('npm_rope') == 1          # behind the one projection GEMM
    (r,) = npm.sim.ropes[ropes:]
    assert (r['heads'], r['pitch'], r['batch'], r['tokens'], r['head_dim'], r['inverse'], r['at'], r['at_lens']) == \
        (heads + kv_heads, (heads + 2 * kv_heads) * 16, 2, 9, 16, 0, 0, 0)
    first, ropes = len(npm.sim.calls), len(npm.sim.ropes)
    att(x, backprop=True, optimizer_=DC.GradRecorder())
    calls = npm.sim.calls[first:]
    (r,) = npm.sim.ropes[ropes:]
    assert (r['heads'], r['pitch'], r['tokens'], r['inverse']) == (heads + kv_heads, (heads + 2 * kv_heads) * 16, 9, 1)
    at = calls.index('npm_rope')
    assert 'npm_mha_core_bwd' in calls[:at] and calls[at + 1] == 'npm_sgemm'      # behind the attention gradient, before dW


def test_separate_tensors_take_two_launches_each_way(npm):
    att, _ = make_mha(npm, 64, 4, 2, seed=5, rope_base=BASE)
    rng = np.random.default_rng(4)
    q, k, v = (rng.standard_normal([2, s, 64]).astype(np.float32) for s in (5, 9, 9))
    ropes = len(npm.sim.ropes)
    att(q, k, v)
    assert not att._packed
    assert [(r['heads'], r['tokens'], r['pitch'], r['inverse']) for r in npm.sim.ropes[ropes:]] == [(4, 5, 64, 0), (2, 9, 32, 0)]
    ropes = len(npm.sim.ropes)
    att(q[:, :5], backprop=True, optimizer_=DC.GradRecorder())
    assert [(r['heads'], r['tokens'], r['pitch'], r['inverse']) for r in npm.sim.ropes[ropes:]] == [(4, 5, 64, 1), (2, 9, 32, 1)]


@pytest.mark.parametrize('kind', ['contiguous', 'paged', 'f16'])
def test_cached_forward_rotates_before_the_append_with_the_mirrors_positions(npm, kind):
    kwargs = dict(contiguous={}, paged=dict(page_size=16), f16=dict(dtype='f16'))[kind]
    append = {'contiguous': 'npm_kv_append', 'paged': 'npm_kv_append_paged', 'f16': 'npm_kv_append_f16'}[kind]
    rng = np.random.default_rng(5)
    x = rng.standard_normal([2, 9, 64]).astype(np.float32)
    uploads = {}
    for base in (None, BASE):
        att, _ = make_mha(npm, 64, 4, 2, seed=6, rope_base=base)
        cache = att.make_cache(2, 32, **kwargs)
        steps = []
        for t, n in ((9, None), (1, None), (3, [3, 1]), (1, [0, 1])):
            first, ropes, ups = len(npm.sim.calls), len(npm.sim.ropes), len(npm.sim.uploads)
            before = cache.lengths.copy()
            att(x[:, :t], cache=cache, new_lengths=n)
            calls = npm.sim.calls[first:]
            steps.append(len(npm.sim.uploads) - ups)
            if base is None:
                assert 'npm_rope' not in calls
                continue
            (r,) = npm.sim.ropes[ropes:]
            assert calls.index('npm_rope') < min(i for i, c in enumerate(calls) if c.startswith('npm_kv_append'))
            assert calls.count(append if n is None or kind != 'contiguous' else 'npm_kv_append_varlen') == 2
            assert (r['heads'], r['tokens'], r['inverse'], r['pitch']) == (6, t, 0, 8 * 16)
            if n is None and kind != 'paged':                             # the scalar call of a uniform contiguous cache
                assert (r['at'], r['at_lens']) == (int(before[0]), 0)
            else:                                                         # the `before` row of the [3, B] mirror the append shares
                assert r['at_lens'] == cache._mirror[1].ptr and cache._mirror[0][0].tolist() == before.tolist()
            assert r['table_rows'] == 32 and att._rope.rows == 32         # sized by make_cache, never grown
        uploads[base] = steps
    assert uploads[BASE] == uploads[None]                                 # not one host-to-device copy more per step


def test_errors(npm):
    with pytest.raises(ValueError, match='even head size'):
        npm.layers.MultiHeadAttention(4, rope_base=BASE)(np.zeros([2, 3, 36], dtype=np.float32))          # Dk 9
    with pytest.raises(ValueError, match='positive'):
        npm.layers.MultiHeadAttention(4, rope_base=0.0)
    with pytest.raises(ValueError, match='odd'):
        npm.device.RopeTable(9, BASE)
    att, _ = make_mha(npm, 64, 4, 2, seed=7, rope_base=BASE)
    kv = np.zeros([2, 5, 64], dtype=np.float32)
    first = len(npm.sim.calls)
    with pytest.raises(NotImplementedError, match='fill_cache'):
        att.fill_cache(att.make_cache(2, 8), kv)
    plain, _ = make_mha(npm, 64, 4, 2, seed=7)
    frozen = plain.fill_cache(plain.make_cache(2, 8), kv)
    first = len(npm.sim.calls)
    with pytest.raises(NotImplementedError, match='frozen'):
        att(kv[:, :2], cache=frozen)
    assert npm.sim.calls[first:] == []                                    # refused before anything is launched
    # Dk != Dv is fine: V is never rotated
    np.random.seed(1)
    wide = npm.layers.MultiHeadAttention(4, rope_base=BASE)
    out = wide(np.zeros([2, 3, 64], dtype=np.float32), np.zeros([2, 3, 64], dtype=np.float32), np.ones([2, 3, 32], dtype=np.float32))
    assert wide._key_dim == 16 and wide._value_dim == 8 and np.asarray(out).shape == (2, 3, 64)


def test_the_entry_point_refuses_bad_arguments(npm):
    """The simulator's restatement of the checks of npm_rope (tests/test_gpu_rope.py holds the real entry point to the same
    list), reached through ``device.rope``: the refusal comes back as an ``NpmError`` with the code."""
    D, _C = npm.device, npm._C
    x = D.zeros([2, 3, 4, 16])
    table = D.RopeTable(16, BASE).ensure(8)
    D.rope(D.Mat(x, 64), 2, 3, 4, 16, table)
    lib = _C.lib()
    args = lambda **kw: [kw.get(k, v) for k, v in (('x', x.ptr), ('pitch', 64), ('batch', 2), ('tokens', 3), ('heads', 4), ('head_dim', 16),
                                                 ('cos', table.cos.ptr), ('sin', table.sin.ptr), ('rows', 8), ('at', 0), ('lens', None),
                                                 ('inverse', 0))]
    assert lib.npm_rope(*args()) == 0
    for bad in (dict(head_dim=15, pitch=60), dict(batch=0), dict(tokens=0), dict(heads=0), dict(rows=0), dict(pitch=63), dict(x=None),
                dict(cos=None), dict(sin=None), dict(at=6), dict(at=-1)):
        assert lib.npm_rope(*args(**bad)) == 10002, bad
    with pytest.raises(_C.NpmError) as err:
        D.rope(D.Mat(x, 60), 2, 3, 4, 16, table)
    assert err.value.code == 10002 and 'npm_rope' in str(err.value)


def test_make_cache_sizes_the_table_once_and_decoding_never_uploads_it_again(npm):
    att, _ = make_mha(npm, 64, 4, 2, seed=8, rope_base=BASE)
    assert att._rope.rows == 2                                            # the first forward: 2 positions
    cache = att.make_cache(2, 40)
    assert att._rope.rows == 64 and att._rope.cos.shape == (64, 8)        # rounded up to a power of two
    tables = att._rope.cos.ptr, att._rope.sin.ptr
    x = npm.device.from_host(np.random.default_rng(6).standard_normal([2, 1, 64]).astype(np.float32))
    ups = len(npm.sim.uploads)
    for _ in range(40):
        att(x, cache=cache)
    assert cache.length == 40 and npm.sim.uploads[ups:] == [] and (att._rope.cos.ptr, att._rope.sin.ptr) == tables
    att(np.zeros([2, 70, 64], dtype=np.float32))                          # a longer training sequence grows it, once
    assert att._rope.rows == 128
    want = RR.tables(128, 16, BASE)
    assert np.array_equal(np.asarray(att._rope.cos), want[0]) and np.array_equal(np.asarray(att._rope.sin), want[1])


# ---- results through the simulator: the checks of tests/test_gpu_rope.py on the restated entry points -----------------------------
@pytest.mark.parametrize('f,heads,kv_heads', [(64, 4, 4), (64, 4, 2), (48, 4, 4)])
def test_layer_forward_and_backward_against_float64(npm, f, heads, kv_heads):
    """B 2, S 9: head size 16 (the fused core) with multi-head and grouped-query attention, head size 12 (the GEMM composition
    and the scalar kernel's shape); output, input gradients and every parameter gradient at BASELINE's 1e-4."""
    RC.check_layer(npm, f, heads, kv_heads, core=(f == 64))


def test_cross_call_counts_each_side_from_zero(npm):
    RC.check_cross(npm)


@pytest.mark.parametrize('norm_first', [True, False])
def test_decoder_and_encoder_keywords(npm, norm_first):
    RC.check_decoder(npm, norm_first)
    RC.check_encoder(npm, norm_first)


@pytest.mark.parametrize('kind', ['contiguous', 'paged', 'f16', 'ragged'])
def test_chunked_decoding_equals_the_whole_causal_forward(npm, kind):
    RC.check_chunked_attention(npm, kind)
    RC.check_chunked_decoder(npm, kind)


def test_the_chunked_reference_is_the_whole_reference():
    rng = np.random.default_rng(3)
    p = {n: a for n, a in __import__('gqa_reference').init_params(rng, 64, 64, 4, 2, scale=0.25).items()}
    p['wo'] = p['wo'].reshape(64, 4, 16)
    x = rng.standard_normal([2, 13, 64])
    want, _ = RR.att_fwd(p, BASE, x, mask=DR.causal_mask(13))
    for sizes in DC.chunkings(13):
        assert_close(RR.mha_cached(p, BASE, DC.split(x, sizes)), want, tol=1e-12, what=f'chunks {sizes[:4]}')


def test_release_and_admit_start_at_position_zero(npm):
    RC.check_release_and_admit(npm)


@pytest.mark.parametrize('f16', [False, True])
def test_prefill_kernel_switches(npm, monkeypatch, f16):
    monkeypatch.setattr(npm.device, 'PREFILL_KERNEL_F16' if f16 else 'PREFILL_KERNEL', True)
    RC.check_prefill_switch(npm, f16)


@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('kind', ['contiguous', 'paged', 'f16'])
def test_stored_rows_are_the_rotated_plain_rows(npm, kind, ragged):
    RC.check_stored_rows(npm, kind, ragged)


def test_off_switch_is_bitwise(npm):
    RC.check_off_switch(npm)


def test_kernel_comparison_runs_on_the_restated_entry_point(npm):
    """The driver of the GPU's bitwise comparison on a thinned grid: the pitched buffer, the guard, the expected rows."""
    rng = np.random.default_rng(5)
    tables = {d: RR.tables(64, d, BASE) for d in RC.VEC_DIMS + RC.SCALAR_DIMS}
    dev = {d: RC.device_tables(npm, t) for d, t in tables.items()}
    for case in RC.kernel_grid()[::37]:
        RC.check_kernel_case(npm, rng, tables, dev, *case)
    x = RC.kernel_rows(rng, 3, 5, 3, 16, 4)
    got = RC.run_rope(npm, x, 3, 16, tables[16], 0, [0, 30, 5], 0, table_rows=32)
    want = RC.expected_rows(x, 3, 16, tables[16], 0, [0, 30, 5], 0, table_rows=32)
    assert np.array_equal(RC.bits(got), RC.bits(want)) and np.array_equal(RC.bits(got[1, 2:]), RC.bits(x[1, 2:]))


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_npm_rope_header_against_bindings(built):
    _C = built
    text = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    assert 'NPM_ABI_VERSION 2' in re.sub(r'\s+', ' ', text)              # an addition: the version stays
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    ctype = {'float *': ctypes.c_void_p, 'const float *': ctypes.c_void_p, 'const int32_t *': ctypes.c_void_p, 'int32_t': ctypes.c_int32,
             'int64_t': ctypes.c_int64}
    args = re.search(r'\bint npm_rope\((.*?)\);', text, flags=re.S).group(1)
    want = [ctype[re.match(r'(.*?)(\w+)$', a.strip()).group(1).strip()] for a in args.split(',')]
    assert len(want) == 12 and _C.SIGNATURES['npm_rope'] == want
    assert hasattr(ctypes.CDLL(_C.LIB_PATH), 'npm_rope'), 'npm_rope not exported'
    bound = _C.load_library()
    count = ctypes.c_int(-1)
    bound.npm_device_count(ctypes.byref(count))
    if count.value == 0:                                                  # no compute without a GPU, as every entry point
        assert bound.npm_rope(None, 0, 0, 0, 0, 0, None, None, 0, 0, None, 0) == 10001
        assert b'npm_rope' in bound.npm_last_error()


def test_the_rope_kernels_use_no_scratch(built):
    """Code-object metadata of the two kernels (tools/kernel_meta.py): no scratch, no spilled register, no LDS."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernel_metadata(os.path.join(os.path.dirname(built.LIB_PATH), 'npm_rope.o'))
    assert sorted(re.search(r'rope_\w+_kernel', n).group(0) for n in meta) == ['rope_scalar_kernel', 'rope_vec_kernel'], list(meta)
    for name, m in meta.items():
        print(name, {k: m[k] for k in ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size')})
        assert m['.vgpr_spill_count'] == m['.sgpr_spill_count'] == m['.private_segment_fixed_size'] == m['.group_segment_fixed_size'] == 0
