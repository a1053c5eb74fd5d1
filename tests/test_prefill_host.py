"""CPU: the prefill attention kernel without a GPU.

* ``prefill_reference.tile_model`` -- float32 in the kernel's accumulation order (16-key tiles in order, online rescale) -- is held
  to HALF of tests/decode_gpu.check's bound on exactly the case grids of tests/test_gpu_prefill.py -- ``kernel_cases``, ``group_cases``
  (partly filled tiles, a second head chunk) and the shifted and saturated scores of ``range_cases`` -- every sequence against
  float64 alone.  Float64 itself is the reference, so it stays inside the GPU bound with room to spare.
* the three entry points: header against bindings and exports.
* dispatch on the simulator of tests/hostsim/ (profile 'prefill').  With ``device.PREFILL_KERNEL`` on, every cached forward the decode kernel
  does not take -- a ragged or paged prefill, a chunk on top of cached rows (uniform contiguous included), a frozen cross cache,
  ``dec.admit`` of a prompt among decoding sequences -- has ``_cached_path == 'prefill'``, records no ``npm_kv_gather_*`` or
  ``npm_mha_mask_summary`` call and no ``npm_d2d`` copy, and uploads nothing but the [3, B] lengths mirror and the block table; a uniform
  contiguous prefill from empty stays on ``'fused_masked'``.  With the switch off the recorded call list is what the simulator
  WITHOUT the new entry points (tests/hostsim/ (profile 'paged')) records for the same schedule; under a split math mode the old path runs.

Every test names npm_mha_prefill_*, ``PREFILL_KERNEL``, ``mha_prefill`` or the path 'prefill': none exists without this feature.
"""

import ctypes
import os
import re

import numpy as np
import pytest

import decode_cases as DC
from hostsim.fixtures import activate, built, deactivate, npm_fixture
import paged_cases as PC
import prefill_reference as PR
import varlen_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_PATH = ('npm_kv_gather_varlen', 'npm_kv_gather_paged', 'npm_mha_mask_summary', 'npm_mha_core_fwd', 'npm_mha_core_fwd_grouped')


npm = npm_fixture('prefill')


@pytest.fixture
def switch_on(npm, monkeypatch):
    monkeypatch.setattr(npm.device, 'PREFILL_KERNEL', True)
    return npm


# ---- the accumulation order in float32 ---------------------------------------------------------------------------------------------
def test_case_grid_covers_what_the_kernel_can_get_wrong():
    cases = PR.kernel_cases()
    assert {c[0] for c in cases} == {16, 32, 64, 128} and {(c[1], c[2]) for c in cases} == set(PR.HEADS)
    assert [PR.tokens_per_block(hq, hkv) for hq, hkv in PR.HEADS] == [64, 16, 8, 32]
    for hq, hkv in PR.HEADS:
        r = PR.tokens_per_block(hq, hkv)
        assert {c[3] for c in cases if (c[1], c[2]) == (hq, hkv)} == {1, 33, r - 1, r, r + 1, 2 * r + 3}
    assert {c[4] for c in cases} == {0, 1} and {c[7] for c in cases} == {False, True}
    assert all(c[5].max() <= 700 + c[3] for c in cases)
    top = [c for c in cases if c[8] == 'top']
    assert any(((c[5] - c[6]) > 0).any() and ((c[5] - c[6]) == 0).any() for c in top)      # a chunk on cached rows beside one from empty
    for d in (16, 32, 64, 128):                                           # every head size sees n = 0, 1, T - 1 and T
        seen = set()
        for c in cases:
            if c[0] == d and c[3] > 2:
                seen |= {('0', '1', 'T-1', 'T')[(0, 1, c[3] - 1, c[3]).index(x)] for x in c[6] if x in (0, 1, c[3] - 1, c[3])}
        assert seen == {'0', '1', 'T-1', 'T'}
    assert any({15, 16, 17} <= set(c[5].tolist()) for c in cases)
    assert all((c[6] <= c[5]).all() for c in cases if c[4])               # causal: the new tokens are among the valid rows


def test_group_grid_covers_partly_filled_tiles_and_a_second_head_chunk():
    """What ``kernel_cases`` cannot reach in mha_prefill_kernel's row mapping: its groupings all divide 64 and none exceeds it."""
    assert all(PR.tile_rows(hq, hkv) == PR.ROWS and PR.head_chunks(hq, hkv) == (1, hq // hkv) for hq, hkv in PR.HEADS)
    cases = PR.group_cases()
    assert 80 <= len(cases) <= 100 and len({PR.case_id(c) for c in cases}) == len(cases)
    assert not {PR.case_id(c) for c in cases} & {PR.case_id(c) for c in PR.kernel_cases()}
    assert {(c[1], c[2]) for c in cases} == set(PR.GROUP_HEADS)
    assert [PR.tile_rows(hq, hkv) for hq, hkv in PR.GROUP_HEADS] == [63, 60, 63, 64, 64]
    assert [PR.head_chunks(hq, hkv) for hq, hkv in PR.GROUP_HEADS] == [(1, 3), (1, 5), (1, 7), (2, 8), (2, 1)]
    partly = [c for c in cases if PR.tile_rows(c[1], c[2]) < PR.ROWS]
    chunked = [c for c in cases if PR.head_chunks(c[1], c[2])[0] > 1]
    assert {PR.tile_rows(c[1], c[2]) for c in partly} == {60, 63}
    assert chunked and all(PR.head_chunks(c[1], c[2])[1] < PR.ROWS for c in chunked)          # the last chunk is partly full
    assert any(c[2] > 1 for c in chunked) and any(c[2] > 1 for c in partly)                   # h = c + gi Hkv with Hkv > 1
    for hq, hkv in PR.GROUP_HEADS:
        r = PR.tokens_per_block(hq, hkv)
        want = {1, r, r + 1, 2 * r + 3} | ({33} if hq // hkv >= PR.ROWS else set())
        assert {c[3] for c in cases if (c[1], c[2]) == (hq, hkv)} == want
    for kind in (partly, chunked):
        assert {c[0] for c in kind} == {16, 32, 64, 128}
        assert {c[4] for c in kind} == {0, 1} and {c[7] for c in kind} == {False, True} and {c[8] for c in kind} == {'top', 'clip'}
        assert any(c[8] == 'clip' and c[5].tolist() == list(PR.EDGE_SET) for c in kind)      # the tile and page edges, and 700
        assert any(c[3] > 2 and {0, 1, c[3] - 1, c[3]} <= set(c[6].tolist()) for c in kind)
    assert PR.EDGE_SET == (15, 16, 17, 64, 65, 700)
    assert all(c[5].max() <= 700 + c[3] for c in cases)
    assert all((c[6] <= c[5]).all() for c in cases if c[4])


def test_range_and_repeat_cases_are_what_the_gpu_tests_need():
    cases = PR.range_cases()
    assert {c[:4] for c in cases} == {(128, 8, 2, 67), (64, 8, 8, 70), (32, 6, 3, 40), (16, 8, 1, 17), (64, 12, 4, 45)}
    assert len(cases) == 5 * 2 * 2 and {c[4:] for c in cases} == {('shift', 0), ('shift', 1), ('saturated', 0), ('saturated', 1)}
    assert (PR.RANGE_BATCH, PR.RANGE_LEN) == (2, 300) and all(c[3] > 32 // (c[1] // c[2]) for c in cases)   # past the decode kernel's rows
    q, k, v, scale = PR.range_data(32, 6, 3, 40, 'saturated')
    assert q.shape == (2, 40, 6, 32) and k.shape == v.shape == (2, 300, 3, 32)
    s = scale * np.einsum('bhd,bjhd->bhj', q[:, 0, :3].astype(np.float64), k.astype(np.float64))
    assert (s.argmax(axis=2) == 299).all()                               # token 0's largest score: the last key, which causal hides
    q, k, v, scale = PR.range_data(32, 6, 3, 40, 'shift')
    s = scale * np.einsum('bthd,bjhd->bthj', q[:, :, :3].astype(np.float64), k.astype(np.float64))
    assert 150 < np.abs(np.median(s, axis=3)).max() <= 210
    reps = PR.repeat_cases()
    assert reps[0][:4] == (128, 8, 2, 2 * PR.tokens_per_block(8, 2) + 3) and any(PR.case_id(c)[:16] == PR.case_id(reps[0])[:16] for c in PR.kernel_cases())
    assert PR.tile_rows(*reps[1][1:3]) < PR.ROWS and PR.head_chunks(*reps[2][1:3])[0] > 1
    for c in reps:
        tiles = {-(-int(x) // PR.TILE) % 2 for x in c[5]}
        assert tiles == {0, 1}, 'an odd and an even number of key tiles'
        assert (c[6] <= c[5]).all() and (c[6] <= c[3]).all()


def _model_fractions(q, k, v, lengths, n, scale, causal, what):
    ctx, lse = PR.tile_model(q, k, v, lengths, n, scale, causal)
    worst_ctx, worst_lse = PR.fractions(ctx, lse, q, k, v, lengths, n, scale, causal)
    print(f'{what}: ctx {worst_ctx:.3f}, lse {worst_lse:.3f} of the GPU bound')
    assert worst_ctx <= 0.5 and worst_lse <= 0.5


@pytest.mark.parametrize('case', PR.group_cases(), ids=PR.case_id)
def test_float32_tile_model_stays_within_half_the_gpu_bound_on_the_group_grid(case):
    d, hq, hkv, t, causal, lengths, n, packed, place = case
    q, k, v = PR.case_data(case)
    _model_fractions(q, k, v, lengths, n, 1.0 / np.sqrt(d), causal, PR.case_id(case))


@pytest.mark.parametrize('case', PR.range_cases(), ids=PR.range_id)
def test_float32_tile_model_stays_within_half_the_gpu_bound_on_shifted_and_saturated_scores(case):
    d, hq, hkv, t, kind, causal = case
    q, k, v, scale = PR.range_data(d, hq, hkv, t, kind)
    _model_fractions(q, k, v, np.full(PR.RANGE_BATCH, PR.RANGE_LEN), None, scale, causal, PR.range_id(case))


@pytest.mark.parametrize('case', PR.kernel_cases(), ids=PR.case_id)
def test_float32_tile_model_stays_within_half_the_gpu_bound(case):
    d, hq, hkv, t, causal, lengths, n, packed, place = case
    q, k, v = PR.case_data(case)
    scale = 1.0 / np.sqrt(d)
    ctx, lse = PR.tile_model(q, k, v, lengths, n, scale, causal)
    worst_ctx, worst_lse = PR.fractions(ctx, lse, q, k, v, lengths, n, scale, causal)
    print(f'{PR.case_id(case)}: ctx {worst_ctx:.3f}, lse {worst_lse:.3f} of the GPU bound')
    assert worst_ctx <= 0.5 and worst_lse <= 0.5


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_prefill_entry_points_header_against_bindings(built):
    _C = built
    text = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint npm_mha_prefill_supported\(int head_dim\);', text)
    assert re.search(r'\bconst char \*npm_last_prefill_kernel\(void\);', text)
    args = re.search(r'\bint npm_mha_prefill_fwd\((.*?)\);', text, flags=re.S).group(1)
    ctype = {'const npm_mha_decode *': ctypes.POINTER(_C.npm_mha_decode), 'const int32_t *': ctypes.c_void_p, 'int32_t': ctypes.c_int32}
    want = [ctype[re.match(r'(.*?)(\w+)$', a.strip()).group(1).strip()] for a in args.split(',')]
    assert len(want) == 6 and _C.SIGNATURES['npm_mha_prefill_fwd'] == want
    assert _C.SIGNATURES['npm_mha_prefill_supported'] == [ctypes.c_int] and _C._SPECIAL['npm_last_prefill_kernel'] == (ctypes.c_char_p, [])
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name in ('npm_mha_prefill_supported', 'npm_mha_prefill_fwd', 'npm_last_prefill_kernel'):
        assert hasattr(lib, name), f'{name} not exported'
    bound = _C.load_library()
    assert [d for d in range(1, 300) if bound.npm_mha_prefill_supported(d)] == [16, 32, 64, 128]
    assert bound.npm_last_prefill_kernel() == b''
    count = ctypes.c_int(-1)
    bound.npm_device_count(ctypes.byref(count))
    if count.value == 0:                                                  # no compute without a GPU, as every entry point
        assert bound.npm_mha_prefill_fwd(ctypes.byref(_C.npm_mha_decode()), None, None, None, 0, 0) == 10001


def test_the_kernel_source_has_one_instance_per_head_size_and_layout(built):
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    names = [n for n in kernel_meta.kernel_metadata(os.path.join(os.path.dirname(built.LIB_PATH), 'npm_prefill.o')) if 'mha_prefill_kernel<' in n]
    assert len(names) == 12
    for d in (16, 32, 64, 128):
        for flags in ('false, false', 'true, false', 'true, true'):
            assert any(f'mha_prefill_kernel<{d}, {flags}>' in n for n in names), (d, flags)


# ---- dispatch --------------------------------------------------------------------------------------------------------------------
def _device_calls(npm, att, x_rows, schedule, cache):
    """The schedule through ``att`` with the chunks already on the device; per call (output, path, calls, uploads)."""
    D = npm.device
    out = []
    for x, n in VR.padded_calls(x_rows, schedule):
        xd = D.from_host(x)
        calls, uploads = len(npm.sim.calls), len(npm.sim.uploads)
        copies = len(npm.sim.copies)
        y = att(xd, cache=cache, new_lengths=n)
        assert npm.sim.copies[copies:] == [], 'npm_d2d: a copy of cache rows'
        out.append((np.asarray(y), att._cached_path, npm.sim.calls[calls:], npm.sim.uploads[uploads:]))
    return out


def _only_lengths_and_table(uploads, batch, cache):
    allowed = {3 * batch * 4} | ({cache.block_table.nbytes} if cache.paged else set())
    assert set(uploads) <= allowed and uploads.count(3 * batch * 4) <= 1, (uploads, allowed)


@pytest.mark.parametrize('heads,kv_heads,f', [(4, 4, 64), (8, 2, 128), (4, 1, 64)])
@pytest.mark.parametrize('page_size', [None, 16, 64])
def test_ragged_prefill_and_second_chunk_run_the_prefill_kernel(switch_on, heads, kv_heads, f, page_size):
    npm = switch_on
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads, batch=3)
    schedule = [np.array(n) for n in ([41, 70, 55], [1, 1, 1], [1, 0, 1], [40, 2, 33], [1, 1, 0])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(1)
    x_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    paged = {} if page_size is None else dict(page_size=page_size, pages=int(sum(PC.pages_of(s, page_size) for s in total)))
    cache = att.make_cache(3, int(total.max()) + 2, **paged)
    assert 3 * 3 * 4 != getattr(cache, 'block_table', np.zeros(0)).nbytes
    runs = _device_calls(npm, att, x_rows, schedule, cache)
    assert [r[1] for r in runs] == ['prefill', 'decode', 'decode', 'prefill', 'decode']
    for _, path, calls, uploads in runs:
        assert not any(c in OLD_PATH for c in calls), calls
        _only_lengths_and_table(uploads, 3, cache)
        if path == 'prefill':
            assert calls.count('npm_mha_prefill_fwd') == 1 and not any('decode_fwd' in c for c in calls)
            want = 'causal=1 varlen=1' + (f' paged={page_size}' if page_size else '')
            assert npm._C.last_prefill_kernel().startswith(f'mha_prefill_kernel D={f // heads} T=') and npm._C.last_prefill_kernel().endswith(want)
    if page_size:
        assert cache.pages_free == 0 and cache.table_uploads <= len(schedule)
    for a, b in zip(VR.collect([r[0] for r in runs], schedule, 3), VR.layer_alone(p, x_rows, schedule)):
        np.testing.assert_allclose(a, b, rtol=2e-6, atol=2e-6)


def test_uniform_contiguous_cache_only_on_top_of_cached_rows(switch_on):
    npm = switch_on
    att, p = DC.make_mha(npm, 64, 4, 2, seed=3, batch=2)
    x = np.random.default_rng(3).standard_normal([2, 90, 64]).astype(np.float32)
    cache = att.make_cache(2, 96)
    runs = _device_calls(npm, att, list(x), [np.array([40, 40]), np.array([1, 1]), np.array([49, 49])], cache)
    assert [r[1] for r in runs] == ['fused_masked', 'decode', 'prefill']          # from empty: the fused forward on the projection
    _, _, calls, uploads = runs[2]
    assert calls.count('npm_mha_prefill_fwd') == 1 and not any(c in OLD_PATH for c in calls) and uploads == []
    assert npm._C.last_prefill_kernel() == 'mha_prefill_kernel D=16 T=49 rows=64 causal=1'   # the scalar call: no length array
    got = np.concatenate([r[0] for r in runs], axis=1)
    for a, b in zip(got, VR.layer_alone(p, list(x), [np.array([40, 40]), np.array([1, 1]), np.array([49, 49])])):
        np.testing.assert_allclose(a, b, rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize('page_size', [None, 16])
@pytest.mark.parametrize('kv_lengths', [None, (75, 2, 33)])
def test_frozen_cross_cache_runs_the_prefill_kernel(switch_on, page_size, kv_lengths):
    """Uniform and ragged memories, contiguous and paged; the uniform contiguous one is longer than the query (the scalar call) in
    one call and shorter in the next (the per-sequence call: the scalar one needs kv_len >= new_tokens)."""
    npm = switch_on
    D = npm.device
    att, p = DC.make_mha(npm, 64, 4, 2, seed=8, batch=3)
    rng = np.random.default_rng(4)
    kv = rng.standard_normal([3, 75, 64]).astype(np.float32)
    lengths = np.full(3, 75) if kv_lengths is None else np.array(kv_lengths)
    paged = {} if page_size is None else dict(page_size=page_size)
    cache = att.fill_cache(att.make_cache(3, 75, **paged), kv, lengths=None if kv_lengths is None else lengths)
    for n in (np.array([40, 0, 17]), np.array([80, 80, 80])):
        x_rows = [rng.standard_normal([s, 64]).astype(np.float32) for s in n]
        (out, path, calls, uploads), = _device_calls(npm, att, x_rows, [n], cache)
        assert path == 'prefill' and calls.count('npm_mha_prefill_fwd') == 1 and not any(c in OLD_PATH for c in calls)
        _only_lengths_and_table(uploads, 3, cache)
        scalar = kv_lengths is None and page_size is None and n.min() == n.max() <= 75
        assert ('varlen=1' in npm._C.last_prefill_kernel()) == (not scalar) and 'causal=0' in npm._C.last_prefill_kernel()
        for got, want, rows in zip(VR.collect([out], [n], 3), VR.cross_alone(p, x_rows, kv, lengths), n):
            if rows:
                np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)
    x = D.from_host(rng.standard_normal([3, 40, 64]).astype(np.float32))
    first = len(npm.sim.calls)
    att(x, cache=cache)
    if kv_lengths is None and page_size is None:
        assert npm._C.last_prefill_kernel() == 'mha_prefill_kernel D=16 T=40 rows=64 causal=0' and npm.sim.calls[first:].count('npm_mha_prefill_fwd') == 1


def _admit_run(npm, dec, q_rows, kv, kv_lengths):
    """tests/paged_cases.py's continuous-batching plan with a 40-token prompt for the fifth sequence; per step (paths, calls)."""
    plan = [np.array(n) for n in ([44, 9, 41, 3, 0], [1, 1, 1, 1, 0], [1, 0, 1, 1, 0], [1, 0, 1, 1, 40], [1, 0, 1, 1, 1])]
    slot = (0, 1, 2, 3, 1)
    state = dec.start_decoding(kv[:4, :23], 64, kv_lengths=kv_lengths[:4], page_size=16, pages=12, memory_capacity=48)
    outs, steps = [], []
    for step, (x5, n5) in enumerate(VR.padded_calls(q_rows, plan)):
        if step == 2:
            state.release(1)
        if step == 3:
            dec.admit(state, 1, kv[4:5], kv_length=int(kv_lengths[4]))
        x, n = np.zeros([4, x5.shape[1], x5.shape[2]], dtype=np.float32), np.zeros(4, dtype=np.int64)
        for seq in range(5):
            if n5[seq]:
                x[slot[seq]], n[slot[seq]] = x5[seq], n5[seq]
        xd = npm.device.from_host(x)
        calls, uploads = len(npm.sim.calls), len(npm.sim.uploads)
        copies = len(npm.sim.copies)
        out = np.asarray(dec.decode(xd, state, new_lengths=n))
        assert npm.sim.copies[copies:] == [], 'npm_d2d: a copy of cache rows'
        steps.append(((dec._self_attention._cached_path, dec._cross_attention._cached_path), npm.sim.calls[calls:], npm.sim.uploads[uploads:]))
        wide = np.zeros((5,) + out.shape[1:], dtype=out.dtype)
        for seq in range(5):
            if n5[seq]:
                wide[seq] = out[slot[seq]]
        outs.append(wide)
    return VR.collect(outs, plan, 5), steps, plan, state


def test_decoder_admit_of_a_prompt_runs_the_prefill_kernel(switch_on):
    npm = switch_on
    f = 64
    dec, p = DC.make_decoder(npm, f, 4, 2, 96, True, True, seed=13, batch=4, seq_kv=23)
    rng = np.random.default_rng(8)
    kv = rng.standard_normal([5, 40, f]).astype(np.float32)
    kv_lengths = np.array([23, 4, 11, 17, 40])
    q_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in (48, 10, 45, 7, 41)]
    got, steps, plan, state = _admit_run(npm, dec, q_rows, kv, kv_lengths)
    assert [s[0] for s in steps] == [('prefill', 'prefill'), ('decode', 'decode'), ('decode', 'decode'), ('prefill', 'prefill'),
                                     ('decode', 'decode')]
    for paths, calls, uploads in steps:
        assert not any(c in OLD_PATH for c in calls), calls
        assert calls.count('npm_mha_prefill_fwd') == (2 if paths[0] == 'prefill' else 0)
        assert set(uploads) <= {3 * 4 * 4, state.self_cache.block_table.nbytes}, uploads
    for a, b in zip(got, VR.decoder_alone(p, q_rows, plan, kv, kv_lengths, True)):
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-5)


def _schedule_calls(npm, seed=2):
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=seed, batch=3)
    schedule = [np.array(n) for n in ([41, 70, 55], [1, 1, 1], [40, 2, 33], [1, 1, 0])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(seed)
    x_rows = [rng.standard_normal([s, 64]).astype(np.float32) for s in total]
    kv = rng.standard_normal([3, 50, 64]).astype(np.float32)
    first, copied = len(npm.sim.calls), len(getattr(npm.sim, 'copies', []))
    outs, paths = [], []
    for kwargs in ({}, dict(page_size=16)):
        cache = att.make_cache(3, int(total.max()) + 2, **kwargs)
        for x, n in VR.padded_calls(x_rows, schedule):
            outs.append(np.asarray(att(x, cache=cache, new_lengths=n)))
            paths.append(att._cached_path)
        uniform = att.make_cache(3, 96, **kwargs)
        for chunk in (40, 1, 45):
            outs.append(np.asarray(att(rng.standard_normal([3, chunk, 64]).astype(np.float32), cache=uniform)))
            paths.append(att._cached_path)
        cross = att.fill_cache(att.make_cache(3, 50, **kwargs), kv, lengths=[50, 3, 20])
        outs.append(np.asarray(att(rng.standard_normal([3, 40, 64]).astype(np.float32), cache=cross)))
        paths.append(att._cached_path)
    return outs, paths, list(npm.sim.calls[first:]), list(npm.sim.uploads), list(getattr(npm.sim, 'copies', [])[copied:])


def test_switch_off_records_the_calls_of_the_simulator_without_the_entry_points(monkeypatch):
    """The switch off (its default) against the simulator WITHOUT npm_mha_prefill_*: the same calls, uploads and outputs."""
    from np_modeling_amd import device as D
    assert D.PREFILL_KERNEL == (os.environ.get('NPM_PREFILL_KERNEL', '0') != '0')
    monkeypatch.setattr(D, 'PREFILL_KERNEL', False)
    runs = []
    for profile in ('paged', 'prefill'):
        npm = activate(profile)
        try:
            assert hasattr(npm.sim, 'npm_mha_prefill_fwd') == (profile == 'prefill')
            runs.append(_schedule_calls(npm))
        finally:
            deactivate()
    (outs_a, paths_a, calls_a, uploads_a, _), (outs_b, paths_b, calls_b, uploads_b, copies) = runs
    assert calls_a == calls_b and uploads_a == uploads_b and paths_a == paths_b
    assert 'prefill' not in paths_b and 'npm_mha_prefill_fwd' not in calls_b and 'npm_mha_prefill_supported' not in calls_b
    assert paths_b.count('fused_masked') == 2 * 5 and any('gather' in c for c in calls_b) and len(copies) == 2 * 3
    for a, b in zip(outs_a, outs_b):
        assert np.array_equal(a, b)


def test_switch_on_replaces_every_fused_masked_call_but_the_uniform_prefill_from_empty(switch_on):
    _, paths, calls, _, copies = _schedule_calls(switch_on)
    half = len(paths) // 2
    assert paths[:half] == ['prefill', 'decode', 'prefill', 'decode', 'fused_masked', 'decode', 'prefill', 'prefill']
    assert paths[half:] == ['prefill', 'decode', 'prefill', 'decode', 'prefill', 'decode', 'prefill', 'prefill']   # paged: always per sequence
    assert not any('gather' in c for c in calls) and copies == []
    assert calls.count('npm_mha_mask_summary') <= 1                      # the uniform prefill from empty builds its causal mask


def test_a_split_math_mode_keeps_the_old_path(switch_on):
    npm = switch_on
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=4, batch=2)
    x = np.random.default_rng(0).standard_normal([2, 40, 64]).astype(np.float32)
    assert npm.device.mha_prefill_supported(16) and not npm.device.mha_prefill_supported(16, 32) and not npm.device.mha_prefill_supported(24)
    npm.set_math('bf16x3')
    try:
        assert not npm.device.mha_prefill_supported(16)
        cache = att.make_cache(2, 96, page_size=16)
        first = len(npm.sim.calls)
        att(x, cache=cache, new_lengths=[40, 7])
        att(x[:, :35], cache=cache, new_lengths=[20, 35])
        assert att._cached_path == 'fused_masked' and 'npm_mha_prefill_fwd' not in npm.sim.calls[first:]
        assert 'npm_kv_gather_paged' in npm.sim.calls[first:]
    finally:
        npm.set_math('f32')
    att(x[:, :33], cache=cache, new_lengths=[4, 33])
    assert att._cached_path == 'prefill'


def test_attend_takes_the_kernel_by_name(switch_on):
    npm = switch_on
    D = npm.device
    cache = D.KVCache(2, 64, 2, 16)
    rows = D.from_host(np.random.default_rng(0).standard_normal([2, 40, 32]).astype(np.float32))
    cache.append(D.Mat(rows, 32), D.Mat(rows, 32), 40)
    q = D.from_host(np.random.default_rng(1).standard_normal([2, 40, 4, 16]).astype(np.float32))
    with pytest.raises(ValueError, match='kernel'):
        cache.attend(D.Mat(q, 64), 4, 40, 0.25, True, kernel='fused')
    with pytest.raises(Exception):
        cache.attend(D.Mat(q, 64), 4, 40, 0.25, True)                      # 80 rows: more than the decode kernel takes
    ctx, lse = cache.attend(D.Mat(q, 64), 4, 40, 0.25, True, want_lse=True, kernel='prefill')
    assert ctx.shape == (2, 40, 4, 16) and lse.shape == (2, 4, 40) and npm.sim.calls[-1] == 'npm_mha_prefill_fwd'
    ctx2, _ = D.mha_prefill(D.Mat(q, 64), cache, 4, 40, 40, 0.25, True)
    assert np.array_equal(np.asarray(ctx), np.asarray(ctx2))
