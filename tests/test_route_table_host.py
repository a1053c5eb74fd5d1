"""CPU: which kernel attends over a key / value cache, and how it is called -- the route table of a cached forward, replayed on
the 'beam' profile of the simulator (tests/hostsim/) against tests/golden/cached_attention_routes.json.

The fixture was recorded BEFORE the attention side of incremental decoding was consolidated into one route decision and one
device call, from the code that still had a ladder per call form.  It is not regenerated: a change of what this file expects is
a change of the path a cached forward takes, of the entry points it calls, of their order or of the host-to-device uploads.

Grid: head shapes (F 64, H 4, Hkv 2) and (F 48, H 4, Hkv 4; no fused kernel) x contiguous / paged (page 16) x f32 / f16 x window
None / 8 x ``PREFILL_KERNEL`` x ``PREFILL_KERNEL_F16``, batch 3, capacity 64.  Each cell runs: prefill T 5, step, ragged chunk
[3, 0, 1], chunk T 17, step, reset, prefill T 40 and -- unwindowed -- a frozen cache of 7 rows queried with T 2 and T 20.  Three
further groups: a split math mode, ``rope_base``, and a forked paged cache with ``SHARED_PREFIX`` on.  Per call the fixture holds
``_cached_path`` (or the exception's type), the entry points in order and the upload byte counts.
"""

import itertools
import json
import os

import numpy as np
import pytest

from hostsim.fixtures import npm_fixture

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cached_attention_routes.json')
BATCH, CAPACITY, PAGE = 3, 64, 16
SHAPES = ((64, 4, 2), (48, 4, 4))
PATHS = ('decode', 'prefill', 'fused_masked', 'gemm', 'decode_shared', 'prefill_shared')


npm = npm_fixture('beam')


def _layer(npm, features, heads, kv_heads, batch, **kwargs):
    np.random.seed(7)
    att = npm.layers.MultiHeadAttention(heads, num_kv_heads=kv_heads, **kwargs)
    att(np.zeros([batch, 2, features], dtype=np.float32))
    for name in ('_wq', '_wk', '_wv', '_wo'):
        arr = getattr(att, name)
        arr.set(np.asarray(arr) * np.float32(2.0 / np.sqrt(features)))
    return att


def _record(npm, att, label, call):
    """[label, path or exception type, entry points, upload byte counts] of one call."""
    sim = npm.sim
    calls, uploads = len(sim.calls), len(sim.uploads)
    try:
        call()
        outcome = 'filled' if label.startswith('fill_cache') else att._cached_path
    except (ValueError, NotImplementedError, RuntimeError) as err:
        outcome = type(err).__name__
    return [label, outcome, list(sim.calls[calls:]), [int(u) for u in sim.uploads[uploads:]]]


def _scenario(npm, att, features, paged, dtype, frozen=True):
    """The scripted calls of one cell; a cache the layer refuses is the cell's only entry."""
    rng = np.random.default_rng(0)
    kwargs = dict(page_size=PAGE) if paged else {}

    def x(tokens):
        return rng.standard_normal([BATCH, tokens, features]).astype(np.float32)

    try:
        cache = att.make_cache(BATCH, CAPACITY, dtype=dtype, **kwargs)
    except (ValueError, NotImplementedError) as err:
        return [['make_cache', type(err).__name__, [], []]]
    out = []
    for label, tokens, n in (('prefill T=5', 5, None), ('step', 1, None), ('ragged chunk [3, 0, 1]', 3, [3, 0, 1]),
                             ('chunk T=17', 17, None), ('step', 1, None), ('reset', 0, None), ('prefill T=40', 40, None)):
        if label == 'reset':
            cache.reset()
            continue
        out.append(_record(npm, att, label, lambda: att(x(tokens), cache=cache, new_lengths=n)))
    if frozen:
        cross = att.make_cache(BATCH, CAPACITY, dtype=dtype, **kwargs)
        out.append(_record(npm, att, 'fill_cache 7', lambda: att.fill_cache(cross, x(7))))
        if cross.frozen:
            for tokens in (2, 20):
                out.append(_record(npm, att, f'frozen T={tokens}', lambda: att(x(tokens), cache=cross)))
    return out


def _switches(monkeypatch, npm, prefill, prefill16):
    monkeypatch.setattr(npm.device, 'PREFILL_KERNEL', bool(prefill))
    monkeypatch.setattr(npm.device, 'PREFILL_KERNEL_F16', bool(prefill16))


def grid_routes(npm, monkeypatch):
    out = {}
    for (f, h, hkv), paged, dtype, window, pk, pk16 in itertools.product(SHAPES, (False, True), ('f32', 'f16'), (None, 8), (0, 1), (0, 1)):
        _switches(monkeypatch, npm, pk, pk16)
        att = _layer(npm, f, h, hkv, BATCH, window=window)
        key = f'F{f} H{h}/{hkv} {"paged" if paged else "contiguous"} {dtype} window={window} prefill={pk} prefill16={pk16}'
        out[key] = _scenario(npm, att, f, paged, dtype, frozen=window is None)
    return out


def split_math_routes(npm, monkeypatch):
    out = {}
    _switches(monkeypatch, npm, 1, 1)
    npm.set_math('bf16x3')
    try:
        for paged, dtype in itertools.product((False, True), ('f32', 'f16')):
            att = _layer(npm, 64, 4, 2, BATCH)
            out[f'bf16x3 {"paged" if paged else "contiguous"} {dtype}'] = _scenario(npm, att, 64, paged, dtype)
    finally:
        npm.set_math('f32')
    return out


def rope_routes(npm, monkeypatch):
    out = {}
    for paged, dtype, window, on in itertools.product((False, True), ('f32', 'f16'), (None, 8), (0, 1)):
        _switches(monkeypatch, npm, on, on)
        att = _layer(npm, 64, 4, 2, BATCH, window=window, rope_base=10000.0)
        out[f'rope {"paged" if paged else "contiguous"} {dtype} window={window} prefill={on}'] = _scenario(npm, att, 64, paged, dtype)
    return out


def forked_routes(npm, monkeypatch):
    """A prompt of 70 rows forked twice on a paged cache (page 16: 64 shared rows), then two steps of the three sequences: T 1 is
    4 score rows per K / V head, T 9 is 36, more than the decode kernel takes."""
    D = npm.device
    out = {}
    _switches(monkeypatch, npm, 1, 1)
    monkeypatch.setattr(D, 'SHARED_PREFIX_MIN_ROWS', PAGE)
    for dtype, tokens, shared in itertools.product(('f32', 'f16'), (1, 9), (False, True)):
        monkeypatch.setattr(D, 'SHARED_PREFIX', shared)
        att = _layer(npm, 128, 8, 2, 4)
        cache = att.make_cache(4, 128, page_size=PAGE, dtype=dtype)
        rng = np.random.default_rng(1)
        steps = [_record(npm, att, 'prompt [70, 0, 0, 0]',
                         lambda: att(rng.standard_normal([4, 70, 128]).astype(np.float32), cache=cache, new_lengths=[70, 0, 0, 0]))]
        cache.fork(0, 1)
        cache.fork(0, 2)
        for _ in range(2):
            steps.append(_record(npm, att, f'forked step T={tokens}',
                                 lambda: att(rng.standard_normal([4, tokens, 128]).astype(np.float32), cache=cache,
                                             new_lengths=[tokens] * 3 + [0])))
        out[f'forked {dtype} T={tokens} shared={int(shared)}'] = steps
    return out


GROUPS = dict(grid=grid_routes, split_math=split_math_routes, rope=rope_routes, forked=forked_routes)


def _fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.mark.parametrize('group', sorted(GROUPS))
def test_cached_forwards_take_the_recorded_routes(npm, monkeypatch, group):
    got, want = GROUPS[group](npm, monkeypatch), _fixture()[group]
    assert sorted(got) == sorted(want)
    for cell in want:
        assert [s[:2] for s in got[cell]] == [s[:2] for s in want[cell]], cell      # the paths first: the shorter message
        for g, w in zip(got[cell], want[cell]):
            assert g == w, (cell, g[0])


def test_the_fixture_holds_every_path_name():
    fixture = _fixture()
    seen = {step[1] for group in fixture.values() for cell in group.values() for step in cell}
    assert set(PATHS) <= seen, sorted(set(PATHS) - seen)
    assert len(fixture['grid']) == 2 * 2 * 2 * 2 * 2 * 2
