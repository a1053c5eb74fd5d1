"""CPU: the prefill attention kernel over half-precision caches without a GPU, on the simulator of tests/hostsim/ (profile 'prefill16').

* routing with ``device.PREFILL_KERNEL_F16`` on: whatever the decode kernel does not take over an fp16 cache -- a prefill from
  empty, a chunk on cached rows, a ragged or paged prefill, a frozen cross cache, the prompt of ``dec.admit`` -- has
  ``_cached_path == 'prefill'``, calls ``npm_mha_prefill_fwd_f16`` once and neither ``npm_kv_gather_f16`` nor the fused forward
  nor ``npm_d2d`` nor an fp32 cache entry point; outputs against float64 attention over the rows AS STORED;
* the switch is independent of ``PREFILL_KERNEL``: off, the calls are the list recorded on the commit before the entry point
  existed (tests/golden/kv16_calls_before_prefill16.json) whatever ``PREFILL_KERNEL`` says; on, the routing is the same with
  ``PREFILL_KERNEL`` on or off;
* a split math mode and an unsupported head size keep their earlier paths;
* ``KVCache.attend(kernel='prefill')`` raises without the switch and runs with it; ``mha_prefill`` always takes the ``_f16`` entry
  point for an fp16 cache;
* no fp32 copy of K / V is allocated: the peak of device memory during a chunk stays below one gathered tensor;
* the entry point: header against bindings and exports, the fp16 instances of the built object.

Every test names ``npm_mha_prefill_fwd_f16`` or ``PREFILL_KERNEL_F16``, and every test but one needs the product's side of them: the
test of the case grid checks the case list of the GPU comparison alone.
"""

import ctypes
import os
import re

import numpy as np
import pytest

import decode_cases as DC
import decode_reference as DR
from hostsim.fixtures import activate, built, deactivate, npm_fixture
import kv16_reference as K16
import varlen_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_CACHE_CALLS = ('npm_kv_append', 'npm_kv_append_varlen', 'npm_kv_append_paged', 'npm_kv_gather_varlen', 'npm_kv_gather_paged',
                   'npm_mha_decode_fwd', 'npm_mha_decode_fwd_varlen', 'npm_mha_decode_fwd_paged', 'npm_mha_prefill_fwd')
OLD_PATH = ('npm_kv_gather_f16', 'npm_mha_mask_summary', 'npm_mha_core_fwd', 'npm_mha_core_fwd_grouped')
ENTRY = 'npm_mha_prefill_fwd_f16'


npm = npm_fixture('prefill16')


@pytest.fixture
def switch_on(npm, monkeypatch):
    monkeypatch.setattr(npm.device, 'PREFILL_KERNEL_F16', True)
    return npm


def _prefill_span(calls):
    """What a call that ran the fp16 prefill kernel may and may not contain."""
    assert calls.count(ENTRY) == 1, calls
    assert not any(c in OLD_PATH or c in F32_CACHE_CALLS for c in calls), calls
    assert 'npm_mha_decode_fwd_f16' not in calls


def _no_read_past_a_length(sim, first, lengths):
    reads = [r for r in sim.f16_reads[first:] if r[0] == 'prefill']
    assert reads and all(take == int(lengths[b]) for _, b, take in reads), (reads, lengths)


# ---- the grid of the GPU's bitwise comparison -----------------------------------------------------------------------------------------
def test_case_grid_of_npm_mha_prefill_fwd_f16_covers_every_axis_value_at_every_head_size():
    """A self-test of the case list of tests/prefill16_reference.py, not of the product: it shows that the GPU comparison meets
    every value of every axis at every head size."""
    import prefill16_reference as P16
    import prefill_reference as PR
    cases = P16.bitwise_cases()
    assert 100 <= len(cases) <= 160 and len({P16.case_id(c) for c in cases}) == len(cases)
    assert [PR.tokens_per_block(hq, hkv) for hq, hkv in P16.HEADS] == [64, 16, 32, 1] and PR.head_chunks(72, 1)[0] == 2
    assert {15, 16, 17, 64, 65} < set(P16.LENGTHS) and max(P16.LENGTHS) >= 300
    for d in (16, 32, 64, 128):
        mine = [c for c in cases if c[0] == d]
        assert {c[1:3] for c in mine} == set(P16.HEADS)
        for hq, hkv in P16.HEADS:
            r = PR.tokens_per_block(hq, hkv)
            assert {c[3] for c in mine if c[1:3] == (hq, hkv)} == {1, r, r + 1, 2 * r + 3}          # 2 r + 3: three token tiles
        assert {c[4] for c in mine} >= set(P16.LENGTHS)
        assert {c[5:] for c in mine} == {(ca, b, lay) for ca in (0, 1) for b in (1, 3) for lay in ('uniform', 'varlen', 'paged16', 'paged64')}
    for c in cases:
        kv, new = P16.lengths(c[6], c[3], c[4], c[7], c[5])
        if kv is None:
            assert c[4] >= c[3]                                           # the uniform call needs kv_len >= new_tokens
        else:
            assert (new <= c[3]).all() and (not c[5] or (new <= kv).all()) and kv.max() == c[4]
            assert c[6] == 1 or (kv[1] == 0 and new[1] == 0 and (c[3] == 1 or new[2] < c[3]))       # no rows; a padded token


# ---- routing ------------------------------------------------------------------------------------------------------------------------
def _chunks(npm, att, x, sizes, cache):
    outs, paths, spans = [], [], []
    for piece in DC.split(x, sizes):
        first, copies, reads = len(npm.sim.calls), len(npm.sim.copies), len(npm.sim.f16_reads)
        outs.append(np.asarray(att(np.ascontiguousarray(piece), cache=cache)))
        paths.append(att._cached_path)
        spans.append(npm.sim.calls[first:])
        assert npm.sim.copies[copies:] == [], 'npm_d2d: a copy of cache rows'
        if paths[-1] == 'prefill':
            _no_read_past_a_length(npm.sim, reads, cache.lengths)
    return outs, paths, spans


def _stored_reference(p, x, sizes, cache_rows):
    """Attention in float64 over K / V AS STORED (``cache_rows``: (k, v) gathered after the last call), per chunk."""
    k, v = (np.asarray(r, dtype=np.float64) for r in cache_rows)
    outs, at = [], 0
    for piece in DC.split(x, sizes):
        t = piece.shape[1]
        q = DR._project(piece.astype(np.float64), p['wq'], p['bq'])
        ctx, _ = DR.decode_attention(q, k, v, at + t, 1.0 / np.sqrt(q.shape[3]), True)
        outs.append(np.einsum('...abc,...dbc->...ad', ctx, p['wo']) + p['bo'])
        at += t
    return outs


@pytest.mark.parametrize('heads,kv_heads,f', [(8, 8, 128), (8, 2, 128), (4, 1, 256)])
@pytest.mark.parametrize('fp32_switch', [False, True])
def test_switch_on_routes_what_the_decode_kernel_leaves_to_npm_mha_prefill_fwd_f16(switch_on, monkeypatch, heads, kv_heads, f, fp32_switch):
    """tests/test_kv16_host.py's chunks 40 (from empty), 1, 3, 40 (on cached rows), 1 with PREFILL_KERNEL_F16 on; PREFILL_KERNEL
    on or off changes nothing."""
    npm = switch_on
    monkeypatch.setattr(npm.device, 'PREFILL_KERNEL', fp32_switch)
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=3)
    sizes = [40, 1, 3, 40, 1]
    x = np.random.default_rng(2).standard_normal([2, sum(sizes), f]).astype(np.float32)
    monkeypatch.setattr(type(att), '_valid_rows', staticmethod(lambda *a: pytest.fail('_valid_rows on an fp16 cache')))
    cache = att.make_cache(2, sum(sizes) + 3, dtype='f16')
    outs, paths, spans = _chunks(npm, att, x, sizes, cache)
    g = heads // kv_heads
    assert paths == ['prefill', 'decode', 'decode' if 3 * g <= 32 else 'prefill', 'prefill', 'decode']
    for path, calls in zip(paths, spans):
        assert calls.count('npm_kv_append_f16') == 2 and not any(c in F32_CACHE_CALLS for c in calls)
        if path == 'decode':
            assert calls.count('npm_mha_decode_fwd_f16') == 1 and ENTRY not in calls and 'npm_kv_gather_f16' not in calls
        else:
            _prefill_span(calls)
    assert npm._C.last_prefill_kernel() == f'mha_prefill_kernel D={f // heads} T=40 rows=64 causal=1 kv=f16'   # the scalar call
    stored = cache.gather(sum(sizes))
    assert np.array_equal(np.asarray(stored[0]), K16.rounded(np.asarray(stored[0])))          # halves, exactly
    for got, want in zip(outs, _stored_reference(p, x, sizes, stored)):
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)


def _f16_schedule(npm):
    """Uniform chunks, a ragged and a paged schedule, a frozen cross cache and a decoder over fp16 caches: (calls, paths, outputs,
    npm_d2d copies)."""
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=4, batch=3)
    dec, _ = DC.make_decoder(npm, 64, 4, 2, 96, True, True, seed=9, batch=3)
    first, copied = len(npm.sim.calls), len(npm.sim.copies)
    rng = np.random.default_rng(1)
    outs, paths = [], []
    for kwargs in ({}, dict(page_size=16)):
        cache = att.make_cache(3, 90, dtype='f16', **kwargs)
        for t, n in ((40, None), (1, None), (3, None), (40, [40, 2, 33]), (1, [1, 0, 1])):
            outs.append(np.asarray(att(rng.standard_normal([3, t, 64]).astype(np.float32), cache=cache, new_lengths=n)))
            paths.append(att._cached_path)
        cross = att.fill_cache(att.make_cache(3, 50, dtype='f16', **kwargs), rng.standard_normal([3, 50, 64]).astype(np.float32),
                               lengths=[50, 3, 20])
        outs.append(np.asarray(att(rng.standard_normal([3, 40, 64]).astype(np.float32), cache=cross)))
        paths.append(att._cached_path)
        state = dec.start_decoding(rng.standard_normal([3, 7, 64]).astype(np.float32), 64, cache_dtype='f16', **kwargs)
        for t in (35, 1):
            outs.append(np.asarray(dec.decode(rng.standard_normal([3, t, 64]).astype(np.float32), state)))
            paths.append((dec._self_attention._cached_path, dec._cross_attention._cached_path))
    return list(npm.sim.calls[first:]), paths, outs, list(npm.sim.copies[copied:])


RECORDED = os.path.join(ROOT, 'tests', 'golden', 'kv16_calls_before_prefill16.json')


def _switch_off_record(npm):
    """What tests/golden/kv16_calls_before_prefill16.json holds: the library calls and ``_cached_path`` of fp16 caches through the
    chunks 40, 1, 3, 40, 1 of tests/test_kv16_host.py's test_layer_attends_to_the_rows_as_stored at its three head groupings (a
    list of calls per chunk), and of ``_f16_schedule``.  The file was recorded by this function on the commit before
    npm_mha_prefill_fwd_f16 existed, on the simulator of tests/hostsim/ (profile 'kv16')."""
    record = {}
    for heads, kv_heads, f in ((8, 8, 128), (8, 2, 128), (4, 1, 256)):
        att, _ = DC.make_mha(npm, f, heads, kv_heads, seed=3)
        sizes = [40, 1, 3, 40, 1]
        x = np.random.default_rng(2).standard_normal([2, sum(sizes), f]).astype(np.float32)
        _, paths, spans = _chunks(npm, att, x, sizes, att.make_cache(2, sum(sizes) + 3, dtype='f16'))
        record[f'chunks H{heads}/{kv_heads}'] = dict(paths=paths, calls=[list(span) for span in spans])
    calls, paths, _, copies = _f16_schedule(npm)
    record['schedule'] = dict(paths=[list(x) if isinstance(x, tuple) else x for x in paths], calls=calls, copies=len(copies))
    return record


def test_switch_off_makes_the_recorded_calls_of_before_npm_mha_prefill_fwd_f16(monkeypatch):
    """PREFILL_KERNEL_F16 off (its default), PREFILL_KERNEL on or off, on the simulator with and without the entry point: the
    calls and paths of fp16 caches are, name for name, the list recorded on the commit before the entry point existed
    (tests/golden/kv16_calls_before_prefill16.json), and the outputs of the runs are equal bit for bit."""
    import json
    from np_modeling_amd import device as D
    assert D.PREFILL_KERNEL_F16 == (os.environ.get('NPM_PREFILL_KERNEL_F16', '0') != '0')
    monkeypatch.setattr(D, 'PREFILL_KERNEL_F16', False)
    with open(RECORDED) as fh:
        recorded = json.load(fh)
    calls = recorded['schedule']['calls']
    assert len(calls) > 100 and ENTRY not in calls and calls.count('npm_kv_gather_f16') == 2 * (2 * 3 + 2 * 2)
    assert recorded['schedule']['paths'].count('fused_masked') == 2 * 3 and recorded['schedule']['copies'] == 0
    assert recorded['chunks H8/2']['paths'] == ['fused_masked', 'decode', 'decode', 'fused_masked', 'decode']
    outs = []
    for profile, fp32_switch in (('kv16', False), ('prefill16', False), ('prefill16', True)):
        monkeypatch.setattr(D, 'PREFILL_KERNEL', fp32_switch)
        npm = activate(profile)
        try:
            assert hasattr(npm.sim, ENTRY) == (profile == 'prefill16')
            assert _switch_off_record(npm) == recorded, (profile, fp32_switch)
            outs.append(_f16_schedule(npm)[2])
        finally:
            deactivate()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)


def test_switch_on_replaces_every_fused_masked_call_over_an_fp16_cache(switch_on):
    """The same schedule with PREFILL_KERNEL_F16 on: no gather, no fused forward, and the decoder needs no change of its own."""
    calls, paths, _, copies = _f16_schedule(switch_on)
    want = ['prefill', 'decode', 'decode', 'prefill', 'decode', 'prefill', ('prefill', 'prefill'), ('decode', 'decode')]
    assert paths == want + want
    assert calls.count(ENTRY) == 2 * (3 + 2) and not any(c in OLD_PATH or c in F32_CACHE_CALLS for c in calls)
    assert copies == []


def test_ragged_and_paged_f16_caches_run_npm_mha_prefill_fwd_f16(switch_on):
    """tests/test_kv16_host.py's ragged schedule, contiguous and paged."""
    npm = switch_on
    att, p = DC.make_mha(npm, 64, 4, 2, seed=4, batch=3)
    schedule = [np.array(n) for n in ([3, 37, 20], [1, 1, 1], [1, 0, 1], [40, 2, 33], [1, 1, 0])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(1)
    x_rows = [rng.standard_normal([s, 64]).astype(np.float32) for s in total]
    runs = []
    for kwargs in ({}, dict(page_size=16)):
        cache = att.make_cache(3, int(total.max()) + 2, dtype='f16', **kwargs)
        first, copies = len(npm.sim.calls), len(npm.sim.copies)
        outs, paths = [], []
        for x, n in VR.padded_calls(x_rows, schedule):
            reads = len(npm.sim.f16_reads)
            outs.append(np.asarray(att(x, cache=cache, new_lengths=n)))
            paths.append(att._cached_path)
            if paths[-1] == 'prefill':
                _no_read_past_a_length(npm.sim, reads, cache.lengths)
                assert npm._C.last_prefill_kernel().endswith('causal=1 varlen=1' + (' paged=16' if kwargs else '') + ' kv=f16')
        calls = npm.sim.calls[first:]
        assert paths == ['prefill', 'decode', 'decode', 'prefill', 'decode']
        assert calls.count('npm_kv_append_f16') == 10 and calls.count(ENTRY) == 2 and calls.count('npm_mha_decode_fwd_f16') == 3
        assert not any(c in OLD_PATH or c in F32_CACHE_CALLS for c in calls) and len(npm.sim.copies) == copies
        assert cache.lengths.tolist() == total.tolist()
        runs.append(outs)
        # float64 over the rows as stored, every sequence alone
        k, v = (np.asarray(r, dtype=np.float64) for r in cache.gather(int(total.max())))
        at = np.zeros(3, dtype=np.int64)
        for (x, n), got in zip(VR.padded_calls(x_rows, schedule), outs):
            at += n
            q = DR._project(x.astype(np.float64), p['wq'], p['bq'])
            ctx, _ = VR.decode_attention(q, k, v, at, n, 0.25, True)
            want = np.einsum('...abc,...dbc->...ad', ctx, p['wo']) + p['bo']
            for i in range(3):
                np.testing.assert_allclose(got[i, :n[i]], want[i, :n[i]], rtol=2e-6, atol=2e-6)
    for a, b in zip(*runs):
        assert np.array_equal(a, b)                                       # paged == contiguous on the simulator too
    cache.release(1)                                                      # paged growth, release and re-admit work on top
    assert cache.lengths.tolist() == [int(total[0]), 0, int(total[2])]
    out = np.asarray(att(rng.standard_normal([3, 34, 64]).astype(np.float32), cache=cache, new_lengths=[1, 34, 0]))
    assert att._cached_path == 'prefill' and np.isfinite(out[0, :1]).all() and np.isfinite(out[1]).all()
    assert cache.lengths.tolist() == [int(total[0]) + 1, 34, int(total[2])]


@pytest.mark.parametrize('page_size', [None, 16])
def test_frozen_cross_caches_run_npm_mha_prefill_fwd_f16(switch_on, page_size):
    """A ragged memory (kv_lengths) under 40 query rows, and a uniform one shorter than the query (the scalar call needs
    kv_len >= new_tokens, so ``KVCache.attend`` takes the per-sequence call, as for an fp32 cache)."""
    npm = switch_on
    att, p = DC.make_mha(npm, 64, 4, 2, seed=8, batch=3)
    rng = np.random.default_rng(4)
    kv = rng.standard_normal([3, 75, 64]).astype(np.float32)
    paged = {} if page_size is None else dict(page_size=page_size)
    tail = f' paged={page_size}' if page_size else ''
    for lengths, rows, scalar in ((np.array([75, 2, 33]), 75, False), (np.full(3, 5), 5, False), (np.full(3, 75), 75, page_size is None)):
        uniform = lengths.min() == lengths.max()
        cache = att.fill_cache(att.make_cache(3, 75, dtype='f16', **paged), kv[:, :rows], lengths=None if uniform else lengths)
        assert cache.frozen and cache.dtype == 'f16'
        x = rng.standard_normal([3, 40, 64]).astype(np.float32)
        first, reads = len(npm.sim.calls), len(npm.sim.f16_reads)
        got = np.asarray(att(x, cache=cache))
        assert att._cached_path == 'prefill'
        _prefill_span(npm.sim.calls[first:])
        assert 'npm_kv_append_f16' not in npm.sim.calls[first:]
        _no_read_past_a_length(npm.sim, reads, lengths)
        assert npm._C.last_prefill_kernel() == 'mha_prefill_kernel D=16 T=40 rows=64 causal=0' + ('' if scalar else ' varlen=1' + tail) + ' kv=f16'
        k, v = (np.asarray(r, dtype=np.float64) for r in cache.gather(rows))
        q = DR._project(x.astype(np.float64), p['wq'], p['bq'])
        ctx, _ = VR.decode_attention(q, k, v, lengths, None, 0.25, False)
        np.testing.assert_allclose(got, np.einsum('...abc,...dbc->...ad', ctx, p['wo']) + p['bo'], rtol=2e-6, atol=2e-6)


def test_split_math_mode_and_other_head_sizes_keep_their_paths(switch_on):
    npm = switch_on
    from np_modeling_amd import _C
    D = npm.device
    att, _ = DC.make_mha(npm, 64, 4, 2, seed=5)
    x = np.random.default_rng(3).standard_normal([2, 40, 64]).astype(np.float32)
    _C.set_math('bf16x3')
    try:
        for kwargs in ({}, dict(page_size=16)):
            cache = att.make_cache(2, 128, dtype='f16', **kwargs)
            first = len(npm.sim.calls)
            att(x, cache=cache)
            att(x[:, :35], cache=cache, new_lengths=[20, 35])
            assert att._cached_path == 'fused_masked' and ENTRY not in npm.sim.calls[first:]
            assert npm.sim.calls[first:].count('npm_kv_gather_f16') == 4
    finally:
        _C.set_math('f32')
    att(x[:, :33], cache=cache, new_lengths=[4, 33])
    assert att._cached_path == 'prefill' and npm.sim.calls[-2] == ENTRY
    # head size 24: make_cache refuses an fp16 cache, and a hand-made one is refused by the layer before anything is launched
    att24, _ = DC.make_mha(npm, 96, 4, 2, seed=6)
    with pytest.raises(NotImplementedError, match='16, 32, 64, 128'):
        att24.make_cache(2, 8, dtype='f16')
    first = len(npm.sim.calls)
    with pytest.raises(NotImplementedError):
        att24(np.zeros([2, 40, 96], dtype=np.float32), cache=D.KVCache(2, 48, 2, 24, dtype='f16'))
    assert ENTRY not in npm.sim.calls[first:] and not D.mha_prefill_supported(24)


def test_attend_takes_npm_mha_prefill_fwd_f16_by_name_only_with_the_switch(npm, monkeypatch):
    D = npm.device
    rng = np.random.default_rng(0)
    rows = D.from_host(rng.standard_normal([2, 40, 32]).astype(np.float32))
    q = D.from_host(rng.standard_normal([2, 40, 4, 16]).astype(np.float32))
    for cache in (D.KVCache(2, 64, 2, 16, dtype='f16'), D.PagedKVCache(2, 64, 2, 16, page_size=16, dtype='f16')):
        cache.append(D.Mat(rows, 32), D.Mat(rows, 32), 40)
        monkeypatch.setattr(D, 'PREFILL_KERNEL_F16', False)
        monkeypatch.setattr(D, 'PREFILL_KERNEL', True)                    # the fp32 switch does not open it
        first = len(npm.sim.calls)
        with pytest.raises(ValueError, match='prefill.*PREFILL_KERNEL_F16'):
            cache.attend(D.Mat(q, 64), 4, 40, 0.25, True, kernel='prefill')
        assert npm.sim.calls[first:] == []
        ctx_low, lse_low = D.mha_prefill(D.Mat(q, 64), cache, 4, 40, 40, 0.25, True, want_lse=True) if not cache.paged else (None, None)
        if not cache.paged:                                               # the low-level call dispatches on the dtype, switch or not
            assert npm.sim.calls[first:] == [ENTRY]
        monkeypatch.setattr(D, 'PREFILL_KERNEL', False)
        monkeypatch.setattr(D, 'PREFILL_KERNEL_F16', True)
        ctx, lse = cache.attend(D.Mat(q, 64), 4, 40, 0.25, True, want_lse=True, kernel='prefill')
        assert ctx.shape == (2, 40, 4, 16) and lse.shape == (2, 4, 40) and npm.sim.calls[-1] == ENTRY
        assert npm._C.last_prefill_kernel().endswith(' kv=f16') and 'npm_mha_prefill_fwd' not in npm.sim.calls
        if not cache.paged:
            assert np.array_equal(np.asarray(ctx), np.asarray(ctx_low)) and np.array_equal(np.asarray(lse), np.asarray(lse_low))
        k, v = (np.asarray(x, dtype=np.float64) for x in cache.gather(40))
        want, want_lse = DR.decode_attention(np.asarray(q), k, v, 40, 0.25, True)
        np.testing.assert_allclose(np.asarray(ctx), want, rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(np.asarray(lse), want_lse, rtol=2e-6, atol=2e-6)


def test_bad_arguments_of_npm_mha_prefill_fwd_f16_are_refused(npm, monkeypatch):
    """``device.mha_prefill`` on an fp16 cache with a descriptor spoilt on its way to the library: the call reaches
    npm_mha_prefill_fwd_f16 and no other entry point, and the refusal comes back as an ``NpmError`` that carries the code and
    names the entry point.  The checks themselves are the simulator's restatement of the entry point's (pitches of 8 halves,
    aligned pointers, a table needs lengths); tests/test_gpu_prefill16.py holds the real entry point to the same list."""
    D, _C = npm.device, npm._C
    rng = np.random.default_rng(2)
    cache = D.KVCache(2, 48, 2, 16, dtype='f16')
    rows = D.from_host(rng.standard_normal([2, 40, 32]).astype(np.float32))
    cache.append(D.Mat(rows, 32), D.Mat(rows, 32), 40)
    q = D.from_host(rng.standard_normal([2, 40, 4, 16]).astype(np.float32))
    table = D.from_host(np.arange(8, dtype=np.float32))                   # any non-NULL address: refused before it is read
    lens = D.from_host(np.zeros(2, dtype=np.float32))
    describe = D._decode_desc

    def call(tweak=None, table=None, page_rows=0, lens=None):
        def spoilt(*args):
            c, ctx, lse, layout = describe(*args)
            if tweak:
                tweak(c)
            if table is not None:
                layout = type('Layout', (), dict(table=table, table_pitch=2, page_rows=page_rows))
            return c, ctx, lse, layout
        monkeypatch.setattr(D, '_decode_desc', spoilt)
        first = len(npm.sim.calls)
        try:
            D.mha_prefill(D.Mat(q, 64), cache, 4, 40, 40, 0.25, True, lens=lens)
            return 0
        except _C.NpmError as e:
            assert ENTRY in str(e)
            return e.code
        finally:
            assert npm.sim.calls[first:] == [ENTRY]

    assert call() == 0
    assert call(lambda c: setattr(c, 'k_pitch', 36)) == 10002             # 4 (mod 8) halves
    assert call(lambda c: setattr(c, 'v_stride_b', 48 * 32 + 4)) == 10002
    assert call(lambda c: setattr(c, 'k', c.k + 2)) == 10002              # a 2-byte offset
    assert call(lambda c: setattr(c, 'head_dim', 48)) == 10003
    assert call(lambda c: setattr(c, 'kv_len', 39)) == 10002              # uniform: kv_len < new_tokens
    assert call(table=table.ptr, page_rows=16) == 10002                   # a table without kv_lens
    for page_rows in (8, 24):
        assert call(table=table.ptr, page_rows=page_rows, lens=(lens.ptr, None)) == 10002


def test_no_fp32_copy_of_the_cache_is_allocated(switch_on, monkeypatch):
    """tests/test_gpu_prefill.py's test_no_gathered_copy_is_allocated on the simulator's allocation counter: one long sequence
    beside short ones in a paged fp16 cache, then a 40-token chunk.  PREFILL_KERNEL_F16 off: K and V of every sequence are
    gathered to the longest as fp32 (two [4, 168, 64] tensors -- more than the fp16 cache itself).  On: the peak of device memory
    during the chunk grows by less than ONE such tensor."""
    npm = switch_on
    D = npm.device
    att, _ = DC.make_mha(npm, 64, 4, 4, seed=5, batch=4)
    rng = np.random.default_rng(5)
    first = rng.standard_normal([4, 128, 64]).astype(np.float32)
    chunk = D.from_host(rng.standard_normal([4, 40, 64]).astype(np.float32))
    one_gathered = 4 * 168 * 64 * 4
    growth = {}
    for switch in (True, False):
        monkeypatch.setattr(D, 'PREFILL_KERNEL_F16', switch)
        cache = att.make_cache(4, 192, page_size=16, pages=16, dtype='f16')
        att(first, cache=cache, new_lengths=[128, 3, 5, 2])
        npm.sim.peak = npm.sim.live
        out = att(chunk, cache=cache, new_lengths=[40, 1, 1, 1])
        growth[switch] = npm.sim.peak - npm.sim.live
        assert att._cached_path == ('prefill' if switch else 'fused_masked') and cache.lengths.tolist() == [168, 4, 6, 3]
        assert np.isfinite(np.asarray(out)).all()
        del cache, out
    print(f'peak above the resting level during the chunk: {growth[True]} bytes with npm_mha_prefill_fwd_f16, {growth[False]} without')
    assert growth[True] < one_gathered and growth[False] >= 2 * one_gathered


def test_decoder_admit_of_a_prompt_over_f16_caches_runs_npm_mha_prefill_fwd_f16(switch_on):
    """A 40-token prompt admitted into the slot a finished sequence gave back, beside sequences that decode single tokens:
    ``TransformerDecoder`` needs nothing of its own, both of its attentions take the kernel."""
    npm = switch_on
    f = 64
    dec, p = DC.make_decoder(npm, f, 4, 2, 96, True, True, seed=13, batch=4, seq_kv=23)
    rng = np.random.default_rng(8)
    kv = rng.standard_normal([5, 40, f]).astype(np.float32)
    kv_lengths = np.array([23, 4, 11, 17, 40])
    state = dec.start_decoding(kv[:4, :23], 64, kv_lengths=kv_lengths[:4], page_size=16, pages=12, memory_capacity=48, cache_dtype='f16')
    steps = [(44, [44, 9, 41, 3]), (1, [1, 1, 1, 1]), (1, [1, 0, 1, 1]), (40, [1, 40, 1, 1]), (1, [1, 1, 1, 1])]
    want = [('prefill', 'prefill'), ('decode', 'decode'), ('decode', 'decode'), ('prefill', 'prefill'), ('decode', 'decode')]
    for step, ((t, n), paths) in enumerate(zip(steps, want)):
        if step == 2:
            state.release(1)
        if step == 3:
            dec.admit(state, 1, kv[4:5], kv_length=40)
        first, copies = len(npm.sim.calls), len(npm.sim.copies)
        out = np.asarray(dec.decode(rng.standard_normal([4, t, f]).astype(np.float32), state, new_lengths=n))
        calls = npm.sim.calls[first:]
        assert (dec._self_attention._cached_path, dec._cross_attention._cached_path) == paths, step
        assert calls.count(ENTRY) == (2 if paths[0] == 'prefill' else 0) and npm.sim.copies[copies:] == []
        assert not any(c in OLD_PATH or c in F32_CACHE_CALLS for c in calls), calls
        assert all(np.isfinite(out[i, :n[i]]).all() for i in range(4))
    assert state.self_cache.dtype == state.cross_cache.dtype == 'f16' and state.positions.tolist() == [48, 41, 45, 7]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_npm_mha_prefill_fwd_f16_header_against_bindings(built):
    _C = built
    text = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    assert 'NPM_ABI_VERSION 2' in re.sub(r'\s+', ' ', text)              # an addition: the version stays
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    ctype = {'const npm_mha_decode *': ctypes.POINTER(_C.npm_mha_decode), 'const int32_t *': ctypes.c_void_p, 'int32_t': ctypes.c_int32}
    args = re.search(r'\bint npm_mha_prefill_fwd_f16\((.*?)\);', text, flags=re.S).group(1)
    want = [ctype[re.match(r'(.*?)(\w+)$', a.strip()).group(1).strip()] for a in args.split(',')]
    assert len(want) == 6 and _C.SIGNATURES[ENTRY] == want == _C.SIGNATURES['npm_mha_prefill_fwd']
    assert hasattr(ctypes.CDLL(_C.LIB_PATH), ENTRY), f'{ENTRY} not exported'
    bound = _C.load_library()
    assert bound.npm_abi_version() == 2
    count = ctypes.c_int(-1)
    bound.npm_device_count(ctypes.byref(count))
    if count.value == 0:                                                  # no compute without a GPU, as every entry point
        assert bound.npm_mha_prefill_fwd_f16(ctypes.byref(_C.npm_mha_decode()), None, None, None, 0, 0) == 10001
        assert b'npm_mha_prefill_fwd_f16' in bound.npm_last_error()       # the error names the entry point that was called


def test_the_object_has_one_f16_instance_per_head_size_and_layout_and_none_spills(built):
    """npm_mha_prefill_fwd_f16's kernels: twelve instances beside the twelve fp32 ones, the same LDS, no scratch."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernel_metadata(os.path.join(os.path.dirname(built.LIB_PATH), 'npm_prefill.o'))
    half = {n: m for n, m in meta.items() if 'mha_prefill_f16_kernel<' in n}
    full = {n: m for n, m in meta.items() if 'mha_prefill_kernel<' in n}
    assert len(half) == 12 and len(full) == 12
    for d in (16, 32, 64, 128):
        for flags in ('false, false', 'true, false', 'true, true'):
            (m16,) = [m for n, m in half.items() if f'mha_prefill_f16_kernel<{d}, {flags}>' in n]
            (m32,) = [m for n, m in full.items() if f'mha_prefill_kernel<{d}, {flags}>' in n]
            assert m16['.vgpr_spill_count'] == m16['.sgpr_spill_count'] == m16['.private_segment_fixed_size'] == 0, (d, flags, m16)
            assert m16['.group_segment_fixed_size'] == m32['.group_segment_fixed_size'] == 2 * 16 * (2 * d + 4) * 4      # fp32 tiles in LDS
