"""CPU: what the key / value caches ASK of the library, call for call, on the simulator of tests/hostsim/ (profile 'paged').

One scripted scenario runs through ``MultiHeadAttention`` with a ``KVCache`` and again with a ``PagedKVCache`` (pages of 16 rows,
a pool smaller than batch x pages per sequence), and a ``TransformerDecoder`` goes through release and admit.  After every step
the entry points called (in order), the byte counts of the host-to-device uploads, the lengths, the block table, the free pages
and the table uploads must equal the lists below.  They were recorded before the cache code was consolidated into one path: a
change of this file's expectations is a change of the order of effects, of the choice of entry point or of the uploads.
"""

import numpy as np
import pytest

import decode_cases as DC
from hostsim.fixtures import npm_fixture

F, HEADS, KV_HEADS, BATCH, CAPACITY = 64, 4, 2, 3, 48
PAGE, POOL = 16, 7                                                        # 3 sequences x 3 pages would be 9


npm = npm_fixture('paged')


class _Trace:
    """Steps of (label, calls, uploads, lengths, block table, pages free, table uploads) since the step before."""

    def __init__(self, sim, cache):
        self.sim, self.cache, self.steps = sim, cache, []
        self.calls, self.uploads = len(sim.calls), len(sim.uploads)

    def step(self, label):
        sim, cache = self.sim, self.cache
        paged = hasattr(cache, 'block_table')
        self.steps.append((label, sim.calls[self.calls:], sim.uploads[self.uploads:], cache.lengths.tolist(),
                           cache.block_table.tolist() if paged else None, cache.pages_free if paged else None,
                           cache.table_uploads if paged else None))
        self.calls, self.uploads = len(sim.calls), len(sim.uploads)


def layer_trace(npm, paged):
    att, _ = DC.make_mha(npm, F, HEADS, KV_HEADS, seed=3, batch=BATCH)
    cache = att.make_cache(BATCH, CAPACITY, page_size=PAGE, pages=POOL) if paged else att.make_cache(BATCH, CAPACITY)
    rng = np.random.default_rng(0)
    trace = _Trace(npm.sim, cache)

    def call(label, tokens, n=None):
        att(rng.standard_normal([BATCH, tokens, F]).astype(np.float32), cache=cache, new_lengths=n)
        trace.step(f'{label}: {att._cached_path}')

    call('prefill T=5', 5)
    call('step', 1)
    call('step', 1)
    call('ragged chunk [3, 0, 1]', 3, [3, 0, 1])
    call('ragged step [1, 1, 0]', 1, [1, 1, 0])
    call('chunk T=17', 17)                                                # 2 x 17 = 34 group rows: more than the decode kernel takes
    if paged:
        cache.release(1)
        trace.step('release(1)')
        call('re-admit [1, 4, 1]', 4, [1, 4, 1])
    cache.reset()
    trace.step('reset')
    return trace.steps


def decoder_trace(npm):
    dec, _ = DC.make_decoder(npm, F, HEADS, KV_HEADS, 96, True, True, seed=5, batch=BATCH, seq_kv=7)
    rng = np.random.default_rng(1)
    kv = rng.standard_normal([BATCH, 7, F]).astype(np.float32)
    first = (len(npm.sim.calls), len(npm.sim.uploads))
    state = dec.start_decoding(kv, CAPACITY, kv_lengths=[7, 3, 5], page_size=PAGE, pages=POOL)
    trace = _Trace(npm.sim, state.self_cache)
    trace.calls, trace.uploads = first
    cross = []

    def step(label):
        trace.step(label)
        cross.append(state.cross_cache.lengths.tolist())

    step('start_decoding')
    dec.decode(rng.standard_normal([BATCH, 4, F]).astype(np.float32), state, new_lengths=[4, 2, 3])
    step('decode [4, 2, 3]')
    state.release(1)
    step('release(1)')
    dec.admit(state, 1, rng.standard_normal([1, 6, F]).astype(np.float32), kv_length=6)
    step('admit(1)')
    dec.decode(rng.standard_normal([BATCH, 3, F]).astype(np.float32), state, new_lengths=[1, 3, 1])
    step('decode [1, 3, 1]')
    return trace.steps, cross


EXPECT_PLAIN = [('prefill T=5: decode', ['npm_sgemm', 'npm_kv_append', 'npm_kv_append', 'npm_mha_decode_fwd', 'npm_sgemm'], [3840], [5, 5, 5],
  None, None, None),
 ('step: decode', ['npm_sgemm', 'npm_kv_append', 'npm_kv_append', 'npm_mha_decode_fwd', 'npm_sgemm'], [768], [6, 6, 6], None,
  None, None),
 ('step: decode', ['npm_sgemm', 'npm_kv_append', 'npm_kv_append', 'npm_mha_decode_fwd', 'npm_sgemm'], [768], [7, 7, 7], None,
  None, None),
 ('ragged chunk [3, 0, 1]: decode',
  ['npm_sgemm', 'npm_kv_append_varlen', 'npm_kv_append_varlen', 'npm_mha_decode_fwd_varlen', 'npm_sgemm'], [2304, 36],
  [10, 7, 8], None, None, None),
 ('ragged step [1, 1, 0]: decode',
  ['npm_sgemm', 'npm_kv_append_varlen', 'npm_kv_append_varlen', 'npm_mha_decode_fwd_varlen', 'npm_sgemm'], [768, 36],
  [11, 8, 8], None, None, None),
 ('chunk T=17: fused_masked',
  ['npm_sgemm', 'npm_kv_append_varlen', 'npm_kv_append_varlen', 'npm_kv_gather_varlen', 'npm_kv_gather_varlen',
   'npm_mha_mask_summary', 'npm_mha_core_fwd_grouped', 'npm_mha_core_fwd', 'npm_sgemm'],
  [13056, 36, 1428], [28, 25, 25], None, None, None),
 ('reset', [], [], [0, 0, 0], None, None, None)]

EXPECT_PAGED = [('prefill T=5: decode', ['npm_sgemm', 'npm_kv_append_paged', 'npm_kv_append_paged', 'npm_mha_decode_fwd_paged', 'npm_sgemm'],
  [3840, 36, 36], [5, 5, 5], [[0, -1, -1], [1, -1, -1], [2, -1, -1]], 4, 1),
 ('step: decode', ['npm_sgemm', 'npm_kv_append_paged', 'npm_kv_append_paged', 'npm_mha_decode_fwd_paged', 'npm_sgemm'],
  [768, 36], [6, 6, 6], [[0, -1, -1], [1, -1, -1], [2, -1, -1]], 4, 1),
 ('step: decode', ['npm_sgemm', 'npm_kv_append_paged', 'npm_kv_append_paged', 'npm_mha_decode_fwd_paged', 'npm_sgemm'],
  [768, 36], [7, 7, 7], [[0, -1, -1], [1, -1, -1], [2, -1, -1]], 4, 1),
 ('ragged chunk [3, 0, 1]: decode',
  ['npm_sgemm', 'npm_kv_append_paged', 'npm_kv_append_paged', 'npm_mha_decode_fwd_paged', 'npm_sgemm'], [2304, 36], [10, 7, 8],
  [[0, -1, -1], [1, -1, -1], [2, -1, -1]], 4, 1),
 ('ragged step [1, 1, 0]: decode',
  ['npm_sgemm', 'npm_kv_append_paged', 'npm_kv_append_paged', 'npm_mha_decode_fwd_paged', 'npm_sgemm'], [768, 36], [11, 8, 8],
  [[0, -1, -1], [1, -1, -1], [2, -1, -1]], 4, 1),
 ('chunk T=17: fused_masked',
  ['npm_sgemm', 'npm_kv_append_paged', 'npm_kv_append_paged', 'npm_kv_gather_paged', 'npm_kv_gather_paged',
   'npm_mha_mask_summary', 'npm_mha_core_fwd_grouped', 'npm_mha_core_fwd', 'npm_sgemm'],
  [13056, 36, 36, 1428], [28, 25, 25], [[0, 3, -1], [1, 4, -1], [2, 5, -1]], 1, 2),
 ('release(1)', [], [], [28, 0, 25], [[0, 3, -1], [-1, -1, -1], [2, 5, -1]], 3, 2),
 ('re-admit [1, 4, 1]: decode',
  ['npm_sgemm', 'npm_kv_append_paged', 'npm_kv_append_paged', 'npm_mha_decode_fwd_paged', 'npm_sgemm'], [3072, 36, 36],
  [29, 4, 26], [[0, 3, -1], [1, -1, -1], [2, 5, -1]], 2, 3),
 ('reset', [], [], [0, 0, 0], [[-1, -1, -1], [-1, -1, -1], [-1, -1, -1]], 7, 3)]

EXPECT_DECODER = [('start_decoding', ['npm_sgemm', 'npm_sgemm', 'npm_kv_append_varlen', 'npm_kv_append_varlen'], [5376, 36], [0, 0, 0],
  [[-1, -1, -1], [-1, -1, -1], [-1, -1, -1]], 7, 0),
 ('decode [4, 2, 3]',
  ['npm_sgemm', 'npm_kv_append_paged', 'npm_kv_append_paged', 'npm_mha_decode_fwd_paged', 'npm_sgemm', 'npm_sgemm',
   'npm_mha_decode_fwd_varlen', 'npm_sgemm', 'npm_sgemm', 'npm_sgemm'],
  [3072, 36, 36, 36], [4, 2, 3], [[0, -1, -1], [1, -1, -1], [2, -1, -1]], 4, 1),
 ('release(1)', [], [], [4, 0, 3], [[0, -1, -1], [-1, -1, -1], [2, -1, -1]], 5, 1),
 ('admit(1)', ['npm_sgemm', 'npm_kv_append', 'npm_sgemm', 'npm_kv_append'], [1536], [4, 0, 3],
  [[0, -1, -1], [-1, -1, -1], [2, -1, -1]], 5, 1),
 ('decode [1, 3, 1]',
  ['npm_sgemm', 'npm_kv_append_paged', 'npm_kv_append_paged', 'npm_mha_decode_fwd_paged', 'npm_sgemm', 'npm_sgemm',
   'npm_mha_decode_fwd_varlen', 'npm_sgemm', 'npm_sgemm', 'npm_sgemm'],
  [2304, 36, 36, 36], [5, 3, 4], [[0, -1, -1], [1, -1, -1], [2, -1, -1]], 4, 2)]

EXPECT_DECODER_CROSS = [[7, 3, 5], [7, 3, 5], [7, 0, 5], [7, 6, 5], [7, 6, 5]]


def _same(got, want):
    assert [s[0] for s in got] == [s[0] for s in want]
    for g, w in zip(got, want):
        assert g == w, g[0]


def test_kvcache_call_and_upload_trace(npm):
    _same(layer_trace(npm, paged=False), EXPECT_PLAIN)


def test_paged_kvcache_call_and_upload_trace(npm):
    _same(layer_trace(npm, paged=True), EXPECT_PAGED)


def test_decoder_release_admit_call_and_upload_trace(npm):
    steps, cross = decoder_trace(npm)
    _same(steps, EXPECT_DECODER)
    assert cross == EXPECT_DECODER_CROSS
