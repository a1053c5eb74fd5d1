"""GPU: the prefill attention kernel over half-precision caches -- npm_mha_prefill_fwd_f16 (csrc/npm_prefill.hip) through the C
ABI, then MultiHeadAttention and TransformerDecoder with ``dtype='f16'`` caches and ``device.PREFILL_KERNEL_F16`` on.

What is held to what:
* the fp16 call equals npm_mha_prefill_fwd of the same layout on a cache holding the rounded values BITWISE, ctx and lse, on the
  grid of tests/prefill16_reference.py (every head size, grouping, token count around the block's tile, length around the key
  tile and the page, layout, causal or not, batch 1 and 3), and so inherits that kernel's float64 bound: the result is also held
  to float64 of the rounded values with ``prefill_reference.fractions`` at the fp32 kernel's own bound (tests/decode_gpu.check's
  formula, fraction <= 1);
* the caches are filled by npm_kv_append_f16; every unwritten half, every unused page and the guard region hold NAN16, the fp32
  cache holds NaN at the same places, table entries past a sequence's last page are -1: a stray read poisons the result;
* edge values (tests/kv16_reference.py EDGE_VALUES) in stored rows come through as their exact fp32 conversions; an inf in V
  behaves as in the fp32 kernel, bitwise;
* refused calls return the documented code and launch nothing;
* the layers: float64 attention over the rows AS STORED (``cache.gather`` after each call) at tests/test_gpu_decode.py's LAYER_TOL,
  and the switch-off run (the fused forward on gathered rows: another summation order) within 2 LAYER_TOL;
* the decoder: a 40-token prompt admitted among decoding sequences, both runs on fp16 caches, held to what
  tests/test_gpu_prefill.py's test of the same name holds: float64 at 1e-4, every sequence alone and the switch-off run at
  2 LAYER_TOL.  The float64 decoder is tests/prefill16_reference.py's ``decoder_alone_stored``: tests/varlen_reference.py's
  ``decoder_alone`` with K / V rounded to fp16 at the point of storage, which is what an fp16 cache attends to; the distance to the
  float64 decoder over UNROUNDED K / V (the storage error of DESIGN.md 4.5b, not the kernel's) is printed beside it.

Every test names ``npm_mha_prefill_fwd_f16`` or ``PREFILL_KERNEL_F16``: none exists without the feature.
"""

import ctypes as C

import numpy as np
import pytest

import decode_cases as DC
import decode_gpu
import decode_reference as DR
import kv16_reference as K16
import paged_cases as PC
import prefill16_reference as P16
import prefill_reference as PR
import varlen_reference as VR
from decode_gpu import GUARD, SENTINEL
from kv16_reference import NAN16

pytestmark = pytest.mark.gpu

LAYER_TOL = 1e-5                  # tests/test_gpu_decode.py: float32 attention + projections at O(1) activations against float64
BAD, UNSUPPORTED = 10002, 10003
ENTRY = 'npm_mha_prefill_fwd_f16'


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


def _lib():
    from np_modeling_amd import _C
    return _C.lib()


# ---- two caches holding the same values: halves written by npm_kv_append_f16, floats placed on the host ------------------------------
class _Caches:
    """K and V of a case in both storage types and one geometry: ``pitch`` elements between rows, ``stride`` between sequences
    (or pages), the rows ``offset`` elements into a wider row.  ``k16`` / ``v16`` / ``k32`` / ``v32`` are device addresses."""

    def __init__(self, k, v, valid, layout, seed, extra=0, offset=0):
        from np_modeling_amd import _C, device as D
        b, cap, hkv, d = k.shape
        self.row, self.pitch, self.offset = hkv * d, hkv * d + extra, offset
        assert self.pitch % 8 == 0 and offset % 8 == 0 and offset + self.row <= self.pitch
        self.valid = np.asarray(valid, dtype=np.int32)
        if layout.startswith('paged'):
            page_rows = int(layout[5:])
            table, pages = K16.paged_table(np.random.default_rng(seed), b, cap, page_rows, spare=3)
            for i in range(b):
                table[i, -(-int(self.valid[i]) // page_rows):] = -1       # entries past the last page are not read
            self.paged, units, per = (table, page_rows), pages, page_rows
        else:
            self.paged, units, per = None, b, cap
        self.stride = per * self.pitch
        self._keep = []
        for name, x in (('k', k), ('v', v)):
            buf, n = K16.half_buffer([units, per, self.pitch], NAN16)
            src = D.from_host(np.ascontiguousarray(x.reshape(b * cap, self.row)))
            at, new = decode_gpu.ints(np.zeros(b, dtype=np.int32)), decode_gpu.ints(self.valid)
            tab = None if self.paged is None else decode_gpu.ints(self.paged[0])
            rc = _lib().npm_kv_append_f16(src.ptr, self.row, buf.ptr + 2 * offset, self.pitch, self.stride, b, cap, self.row, 0, at.ptr, new.ptr,
                                          None if tab is None else tab.ptr, 0 if tab is None else self.paged[0].shape[1],
                                          0 if tab is None else self.paged[1])
            _C.check(rc, 'npm_kv_append_f16')
            want16 = self._place(K16.to_f16(x).view(np.uint16), np.uint16(NAN16), units, per)
            bits = buf.numpy().view(np.uint16)
            assert np.array_equal(bits[:n], want16.ravel()) and (bits[n:] == NAN16).all(), 'npm_kv_append_f16 wrote something else'
            f32 = D.from_host(self._place(K16.rounded(x), np.float32(np.nan), units, per))
            self._keep += [buf, f32]
            setattr(self, name + '16', buf.ptr + 2 * offset)
            setattr(self, name + '32', f32.ptr + 4 * offset)

    def _place(self, x, fill, units, per):
        """``x`` [B, cap, Hkv, D] -> [units, per, pitch] holding the valid rows where the cache has them and ``fill`` elsewhere."""
        out = np.full([units, per, self.pitch], fill, dtype=x.dtype)
        lo, hi = self.offset, self.offset + self.row
        for i, length in enumerate(self.valid):
            rows = x[i, :length].reshape(length, self.row)
            if self.paged is None:
                out[i, :length, lo:hi] = rows
            else:
                table, page_rows = self.paged
                for first in range(0, int(length), page_rows):
                    take = min(page_rows, int(length) - first)
                    out[table[i, first // page_rows], :take, lo:hi] = rows[first:first + take]
        return out


def _call(entry, q, kptr, vptr, pitch, stride, hkv, lmax, scale, causal, kv_lens=None, new_lens=None, paged=None, expect=0, tweak=None):
    """``entry`` (npm_mha_prefill_fwd or npm_mha_prefill_fwd_f16) -> ctx [B, T, Hq, D], lse [B, Hq, T], kernel string.  ``expect``:
    the call must return that code and leave ctx and lse at their sentinels."""
    from np_modeling_amd import _C, device as D
    b, t, hq, d = q.shape
    qd = D.from_host(q)
    ctx = D.full([b * t * hq * d + GUARD], SENTINEL)
    lse = D.full([b * hq * t + GUARD], SENTINEL)
    c = _C.npm_mha_decode()
    c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim = b, hq, hkv, t, lmax, d
    c.causal, c.scale = int(causal), scale
    c.q, c.q_pitch = qd.ptr, hq * d
    c.k, c.k_pitch, c.k_stride_b = kptr, pitch, stride
    c.v, c.v_pitch, c.v_stride_b = vptr, pitch, stride
    c.ctx, c.ctx_pitch, c.lse = ctx.ptr, hq * d, lse.ptr
    if tweak is not None:
        tweak(c)
    lens = None if kv_lens is None else decode_gpu.ints(kv_lens)
    new = None if new_lens is None else decode_gpu.ints(new_lens)
    table, table_pitch, page_rows = (None, 0, 0) if paged is None else (decode_gpu.ints(paged[0]), paged[0].shape[1], paged[1])
    rc = getattr(_lib(), entry)(C.byref(c), None if lens is None else lens.ptr, None if new is None else new.ptr,
                                None if table is None else table.ptr, table_pitch, page_rows)
    if expect:
        assert rc == expect, (rc, _lib().npm_last_error())
        assert entry.encode() in _lib().npm_last_error(), 'the error names the entry point that was called'
        np.testing.assert_array_equal(ctx.numpy(), SENTINEL)              # nothing was launched
        np.testing.assert_array_equal(lse.numpy(), SENTINEL)
        return None
    _C.check(rc, entry)
    return (decode_gpu.guarded(ctx, b * t * hq * d).reshape(b, t, hq, d), decode_gpu.guarded(lse, b * hq * t).reshape(b, hq, t),
            _C.last_prefill_kernel())


def _both(q, caches, hkv, lmax, scale, causal, kv_lens, new_lens):
    got = _call(ENTRY, q, caches.k16, caches.v16, caches.pitch, caches.stride, hkv, lmax, scale, causal, kv_lens, new_lens, caches.paged)
    want = _call('npm_mha_prefill_fwd', q, caches.k32, caches.v32, caches.pitch, caches.stride, hkv, lmax, scale, causal, kv_lens, new_lens,
                 caches.paged)
    return got, want


def _bits_equal(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f'{what}: ctx differs from the fp32 kernel on the rounded values'
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f'{what}: lse differs from the fp32 kernel on the rounded values'


# ---- 1. bitwise against npm_mha_prefill_fwd on the rounded values, and float64 at that kernel's bound -----------------------------------
@pytest.mark.parametrize('case', P16.bitwise_cases(), ids=P16.case_id)
def test_npm_mha_prefill_fwd_f16_equals_the_f32_kernel_on_the_rounded_values_bitwise(npm, case):
    d, hq, hkv, t, length, causal, b, layout = case
    q, k, v = decode_gpu.data(d * 7 + hq + t + length + causal, b, t, hq, hkv, d, length + 5)
    kv_lens, new_lens = P16.lengths(b, t, length, layout, causal)
    valid = np.full(b, length, dtype=np.int32) if kv_lens is None else kv_lens
    if new_lens is not None:
        q[np.arange(t)[None, :] >= new_lens[:, None]] = np.nan            # padded query rows are never read into a result
    scale = 1.0 / np.sqrt(d)
    caches = _Caches(k, v, valid, layout, seed=length + d)
    got, want = _both(q, caches, hkv, length, scale, causal, kv_lens, new_lens)
    tail = {'uniform': '', 'varlen': ' varlen=1', 'paged16': ' varlen=1 paged=16', 'paged64': ' varlen=1 paged=64'}[layout]
    assert want[2] == f'mha_prefill_kernel D={d} T={t} rows={PR.ROWS} causal={causal}{tail}' and got[2] == want[2] + ' kv=f16'
    _bits_equal(got, want, f'{got[2]} L={valid.tolist()}')
    n = np.full(b, t) if new_lens is None else new_lens
    worst_ctx, worst_lse = PR.fractions(got[0], got[1], np.nan_to_num(q), K16.rounded(k), K16.rounded(v), valid, n, scale, causal)
    print(f'{got[2]} L={valid.tolist()}: ctx {worst_ctx:.3f}, lse {worst_lse:.3f} of the fp32 kernel\'s float64 bound')
    assert worst_ctx <= 1.0 and worst_lse <= 1.0


@pytest.mark.parametrize('d,hq,hkv', [(16, 8, 1), (128, 6, 3)])
@pytest.mark.parametrize('layout', ['uniform', 'paged16'])
def test_npm_mha_prefill_fwd_f16_inside_a_wider_row(npm, d, hq, hkv, layout):
    """K / V of the call sit 8 (D 16: 24) halves into rows that are 24 (40) halves wider than Hkv D: a pitch that is a multiple
    of 8 halves and not of the row, a pointer that is 16-byte aligned and not at the start of the buffer."""
    b, t, length = 3, 70, 81
    q, k, v = decode_gpu.data(d + hq, b, t, hq, hkv, d, length)
    valid = np.array([81, 70, 75], dtype=np.int32)
    extra, offset = (40, 24) if d == 16 else (24, 8)
    caches = _Caches(k, v, valid if layout != 'uniform' else np.full(b, length), layout, seed=d, extra=extra, offset=offset)
    assert caches.pitch % 8 == 0 and caches.pitch % caches.row
    kv_lens = None if layout == 'uniform' else valid
    got, want = _both(q, caches, hkv, length, 1.0 / np.sqrt(d), 1, kv_lens, None)
    _bits_equal(got, want, got[2])
    lens = np.full(b, length) if kv_lens is None else valid
    assert max(PR.fractions(got[0], got[1], q, K16.rounded(k), K16.rounded(v), lens, np.full(b, t), 1.0 / np.sqrt(d), 1)) <= 1.0


@pytest.mark.parametrize('case', [(128, 8, 2, 35, (304, 512, 17), (35, 35, 17)), (16, 72, 1, 5, (65, 320, 5), (5, 4, 5))])
def test_npm_mha_prefill_fwd_f16_repeated_alone_and_paged_is_bitwise_equal(npm, case):
    """The identities the fp32 kernel has, on the fp16 instance itself: the same call three times (the tiles are double buffered in
    LDS behind one barrier per tile), paged against contiguous, a sequence in a batch against that sequence alone."""
    d, hq, hkv, t, lengths, n = case
    lengths, n = np.array(lengths, dtype=np.int32), np.array(n, dtype=np.int32)
    lmax, scale = int(lengths.max()), 1.0 / np.sqrt(d)
    q, k, v = decode_gpu.data(d + t, 3, t, hq, hkv, d, lmax + 3)
    flat = _Caches(k, v, lengths, 'varlen', seed=1)
    first = _call(ENTRY, q, flat.k16, flat.v16, flat.pitch, flat.stride, hkv, lmax, scale, 1, lengths, n)
    for repeat in (1, 2):
        _bits_equal(first, _call(ENTRY, q, flat.k16, flat.v16, flat.pitch, flat.stride, hkv, lmax, scale, 1, lengths, n), f'run {repeat}')
    for layout in ('paged16', 'paged64'):
        pool = _Caches(k, v, lengths, layout, seed=d)
        _bits_equal(first, _call(ENTRY, q, pool.k16, pool.v16, pool.pitch, pool.stride, hkv, lmax, scale, 1, lengths, n, pool.paged), layout)
    for i in range(3):
        one = _Caches(k[i:i + 1], v[i:i + 1], lengths[i:i + 1], 'varlen', seed=2)
        alone = _call(ENTRY, q[i:i + 1], one.k16, one.v16, one.pitch, one.stride, hkv, int(lengths[i]), scale, 1, lengths[i:i + 1], n[i:i + 1])
        _bits_equal((first[0][i:i + 1], first[1][i:i + 1]), alone, f'sequence {i} alone')


# ---- 2. edge values ------------------------------------------------------------------------------------------------------------------
def test_npm_mha_prefill_fwd_f16_edge_values_come_through_exactly(npm):
    """D 16: a row of V is the row of edge values.  A causal prefill from empty: token 0 (a zero query) sees key 0 alone, so its ctx
    IS V[0] as stored (p = 1, l = 1) -- the largest finite half, subnormals, what rounds to zero -- for every query head.  K holds the
    same row at key 1 (scores up to 65504 |q|: the softmax saturates, nothing overflows); an inexact conversion of it would show
    against the fp32 kernel, which is handed the exact values.  Then an inf in V at a key rows 0 .. 4 do not see and the later ones
    do: whatever the fp32 kernel makes of it (inf, and NaN from 0 inf inside the shared tile), bit for bit."""
    d, hq, hkv, t, b = 16, 4, 2, 40, 2
    q, k, v = decode_gpu.data(5, b, t, hq, hkv, d, t)
    finite = K16.EDGE_VALUES.copy()
    finite[np.isinf(K16.rounded(finite))] = 0.25
    v[:, 0, :, :] = finite
    k[:, 1, 0, :] = finite
    q[:, 0] = 0.0                                                         # token 0: score 0, p = exp2(0) = 1, l = 1, ctx = 1 V[0] / 1
    scale = 0.25
    caches = _Caches(k, v, np.full(b, t), 'uniform', seed=0)
    got, want = _both(q, caches, hkv, t, scale, 1, None, None)
    _bits_equal(got, want, 'edge values in K and V')
    assert np.isfinite(got[0]).all()
    stored = K16.rounded(finite)
    assert stored[0] == 65504.0 and stored[5] == np.float32(17 * 2.0 ** -24) and stored[6] == np.float32(2.0 ** -24) and stored[7] == 0.0
    for h in range(hq):
        assert np.array_equal(got[0][:, 0, h], np.broadcast_to(stored, (b, d))), f'head {h}: V[0] did not come through exactly'
    # inf in V (K without the edge row: no weight underflows to 0, so a row that sees key 5 gets inf, not 0 inf)
    k = decode_gpu.data(6, b, t, hq, hkv, d, t)[1]
    v[:, 5, 0, 3] = 65520.0                                               # rounds to inf
    v[:, 5, 1, 7] = -1e6
    caches = _Caches(k, v, np.full(b, t), 'uniform', seed=0)
    got, want = _both(q, caches, hkv, t, scale, 1, None, None)
    _bits_equal(got, want, 'inf in V')
    assert np.isposinf(got[0][:, 5:, 0, 3]).all() and np.isneginf(got[0][:, 5:, 1, 7]).all()   # the rows that see key 5
    assert np.isfinite(got[0][:, :, :, 0]).all()                          # the other columns never meet it


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_npm_mha_prefill_fwd_f16_bad_arguments_launch_nothing(npm):
    b, t, hq, hkv, d, length = 2, 40, 4, 2, 32, 48
    row = hkv * d
    q, k, v = decode_gpu.data(2, b, t, hq, hkv, d, length)
    lens = np.array([48, 44], dtype=np.int32)
    flat = _Caches(k, v, lens, 'varlen', seed=0)
    pool = _Caches(k, v, lens, 'paged16', seed=0)
    table = pool.paged[0]
    assert _call(ENTRY, q, flat.k16, flat.v16, row, flat.stride, hkv, length, 0.2, 1, lens, None)[2].endswith('varlen=1 kv=f16')

    def bad(expect=BAD, caches=flat, kv_lens=lens, paged=None, lmax=length, **fields):
        def tweak(c):
            for name, value in fields.items():
                setattr(c, name, value(c) if callable(value) else value)
        _call(ENTRY, q, caches.k16, caches.v16, row, caches.stride, hkv, lmax, 0.2, 1, kv_lens, None, paged, expect=expect, tweak=tweak)

    bad(k_pitch=row + 4)                                                  # a pitch of 4 (mod 8) halves: fine for floats, not for halves
    bad(v_pitch=row + 4)
    bad(k_stride_b=flat.stride + 4)
    bad(k=lambda c: c.k + 2)                                              # a 2-byte offset
    bad(k=lambda c: c.k + 8)                                              # 4 halves: aligned for a half4, not for the 16-byte piece
    bad(v=lambda c: c.v + 2)
    bad(caches=pool, kv_lens=None, paged=(table, 16))                     # a table without kv_lens
    for page_rows in (8, 24):
        bad(caches=pool, paged=(table, page_rows))
    bad(caches=pool, paged=(table, 16), lmax=16 * table.shape[1] + 1)     # the table rows are shorter than d->kv_len needs
    bad(kv_lens=None, lmax=t - 1)                                         # uniform: kv_len < new_tokens
    bad(heads=3)
    bad(scale=0.0)
    bad(q=lambda c: c.q + 4)
    for size in (8, 48, 256):
        bad(expect=UNSUPPORTED, head_dim=size)


# ---- 4. MultiHeadAttention, switch on ------------------------------------------------------------------------------------------------
@pytest.fixture
def switch(npm, monkeypatch):
    def set_switch(on):
        monkeypatch.setattr(npm.device, 'PREFILL_KERNEL_F16', on)
    return set_switch


def _stored_step(p, x, cache, n, causal=True):
    """float64 attention of the chunk ``x`` [B, T, F] (sequence b brings n[b] tokens, already appended) over the rows AS STORED."""
    k, v = (np.asarray(r, dtype=np.float64) for r in cache.gather(max(cache.max_length, 1)))
    q = DR._project(np.asarray(x, dtype=np.float64), p['wq'], p['bq'])
    ctx, _ = VR.decode_attention(q, k, v, cache.lengths, n, 1.0 / np.sqrt(q.shape[3]), causal)
    return np.einsum('...abc,...dbc->...ad', ctx, p['wo']) + p['bo']


def _schedule_run(att, p, x_rows, schedule, capacity, want_paths, tail, **paged):
    """The schedule through ``att`` with a fresh fp16 cache; every call against float64 over the rows as stored at LAYER_TOL."""
    from np_modeling_amd import _C
    cache = att.make_cache(len(x_rows), capacity, dtype='f16', **paged)
    outs = []
    for step, (x, n) in enumerate(VR.padded_calls(x_rows, schedule)):
        got = np.asarray(att(x, cache=cache, new_lengths=n))
        assert att._cached_path == want_paths[step], (step, att._cached_path)
        if att._cached_path == 'prefill':
            assert _C.last_prefill_kernel().endswith(tail + ' kv=f16'), _C.last_prefill_kernel()
        want = _stored_step(p, x, cache, n)
        for i in range(len(x_rows)):
            if n[i]:
                decode_gpu.layer_close(got[i, :n[i]], want[i, :n[i]], LAYER_TOL, f'step {step} sequence {i} ({att._cached_path}) vs float64 of the stored rows')
        outs.append(got)
    assert cache.lengths.tolist() == VR.schedule_rows(schedule).tolist()
    return outs, cache


@pytest.mark.parametrize('heads,kv_heads,f', [(8, 2, 512), (6, 3, 192), (5, 1, 160)])
@pytest.mark.parametrize('page_size', [16, 64])
def test_layer_ragged_prefill_and_second_chunk_with_PREFILL_KERNEL_F16(npm, switch, heads, kv_heads, f, page_size):
    """tests/test_gpu_prefill.py's schedule into a paged fp16 cache: a ragged prompt of 41 .. 70 tokens, single tokens, a second
    chunk on top, single tokens."""
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads + f, batch=3)
    schedule = [np.array(n) for n in ([41, 70, 55], [1, 1, 1], [1, 0, 1], [40, 2, 33], [1, 1, 0])]
    total = VR.schedule_rows(schedule)
    rng = np.random.default_rng(f)
    x_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    pages = int(sum(PC.pages_of(s, page_size) for s in total))
    kwargs = dict(page_size=page_size, pages=pages)
    tail = f'causal=1 varlen=1 paged={page_size}'
    switch(False)
    off, _ = _schedule_run(att, p, x_rows, schedule, int(total.max()) + 5, ['fused_masked', 'decode', 'decode', 'fused_masked', 'decode'], tail, **kwargs)
    switch(True)
    got, cache = _schedule_run(att, p, x_rows, schedule, int(total.max()) + 5, ['prefill', 'decode', 'decode', 'prefill', 'decode'], tail, **kwargs)
    assert cache.pages_in_use == pages and cache.pages_free == 0
    stored = np.asarray(cache.gather(cache.max_length)[0])
    assert np.array_equal(stored, K16.rounded(stored))                    # what the cache holds are halves
    for i, (a, c) in enumerate(zip(VR.collect(got, schedule, 3), VR.collect(off, schedule, 3))):
        decode_gpu.layer_close(a, c, 2 * LAYER_TOL, f'paged {page_size} H{heads}/{kv_heads} sequence {i} vs PREFILL_KERNEL_F16 off')


@pytest.mark.parametrize('heads,kv_heads,f,below,above', [(4, 4, 256, 32, 33), (4, 1, 512, 8, 9), (12, 4, 192, 10, 11)])
def test_layer_hands_over_from_decode_to_npm_mha_prefill_fwd_f16_past_32_rows(npm, switch, heads, kv_heads, f, below, above):
    """A uniform contiguous fp16 cache with the switch on: the prompt from empty is the prefill kernel's (an fp16 cache is attended
    to as stored), (Hq / Hkv) T <= 32 the decode kernel's, one more row the prefill kernel's again (its scalar call)."""
    from np_modeling_amd import _C
    switch(True)
    att, p = DC.make_mha(npm, f, heads, kv_heads, seed=heads + below, batch=2)
    sizes = [40, below, above]
    x = np.random.default_rng(f + below).standard_normal([2, sum(sizes), f]).astype(np.float32)
    cache = att.make_cache(2, sum(sizes) + 3, dtype='f16')
    for piece, path in zip(DC.split(x, sizes), ['prefill', 'decode', 'prefill']):
        t = piece.shape[1]
        got = np.asarray(att(np.ascontiguousarray(piece), cache=cache))
        assert att._cached_path == path
        if path == 'prefill':
            assert _C.last_prefill_kernel() == f'mha_prefill_kernel D={f // heads} T={t} rows={PR.ROWS} causal=1 kv=f16'
        decode_gpu.layer_close(got, _stored_step(p, piece, cache, np.full(2, t)), LAYER_TOL, f'H{heads}/{kv_heads} {path} chunk of {t}')


@pytest.mark.parametrize('page_size', [None, 16])
@pytest.mark.parametrize('kind', ['kv_lengths', 'short'])
def test_layer_frozen_cross_f16_cache_with_PREFILL_KERNEL_F16(npm, switch, page_size, kind):
    """A ragged memory of 75 / 2 / 33 rows under 40 / 0 / 17 query rows, and a uniform memory of 5 rows under 40 query rows (the
    scalar call needs kv_len >= new_tokens: ``KVCache.attend`` takes the per-sequence call)."""
    from np_modeling_amd import _C
    att, p = DC.make_mha(npm, 256, 8, 2, seed=8, batch=3)
    rng = np.random.default_rng(4)
    if kind == 'kv_lengths':
        kv, kv_lengths, n = rng.standard_normal([3, 75, 256]).astype(np.float32), np.array([75, 2, 33]), np.array([40, 0, 17])
    else:
        kv, kv_lengths, n = rng.standard_normal([3, 5, 256]).astype(np.float32), None, np.array([40, 40, 40])
    x = rng.standard_normal([3, 40, 256]).astype(np.float32)
    x[np.arange(40)[None, :] >= n[:, None]] = 0.0
    paged = {} if page_size is None else dict(page_size=page_size)
    outs = []
    for on in (False, True):
        switch(on)
        cache = att.fill_cache(att.make_cache(3, kv.shape[1], dtype='f16', **paged), kv, lengths=kv_lengths)
        outs.append(np.asarray(att(x, cache=cache, new_lengths=None if kind == 'short' else n)))
        assert att._cached_path == ('prefill' if on else 'fused_masked')
    assert _C.last_prefill_kernel() == f'mha_prefill_kernel D=32 T=40 rows={PR.ROWS} causal=0 varlen=1' + (f' paged={page_size}' if page_size else '') + ' kv=f16'
    want = _stored_step(p, x, cache, n, causal=False)
    for i in range(3):
        if n[i]:
            decode_gpu.layer_close(outs[1][i, :n[i]], want[i, :n[i]], LAYER_TOL, f'cross {kind} sequence {i} vs float64 of the stored rows')
            decode_gpu.layer_close(outs[1][i, :n[i]], outs[0][i, :n[i]], 2 * LAYER_TOL, f'cross {kind} sequence {i} vs PREFILL_KERNEL_F16 off')


def test_no_fp32_copy_is_allocated_with_PREFILL_KERNEL_F16(npm, switch):
    """tests/test_gpu_prefill.py's test_no_gathered_copy_is_allocated over an fp16 cache: one long sequence beside short ones,
    then a 40-token chunk.  Switch off: K and V of every sequence are gathered to the longest as fp32 ([4, 552, 256] floats
    each).  Switch on: the pool grows by less than ONE such tensor."""
    from np_modeling_amd import device as D
    att, _ = DC.make_mha(npm, 256, 4, 4, seed=5, batch=4)
    rng = np.random.default_rng(5)
    first = rng.standard_normal([4, 512, 256]).astype(np.float32)
    chunk = rng.standard_normal([4, 40, 256]).astype(np.float32)
    one_gathered = 4 * 552 * 256 * 4
    growth = {}
    for on in (True, False):
        switch(on)
        cache = att.make_cache(4, 600, page_size=64, pages=12, dtype='f16')
        att(first, cache=cache, new_lengths=[512, 3, 5, 2])
        D.synchronize()
        D.trim_pool()
        before = D.pool_stats()[1]
        out = np.asarray(att(chunk, cache=cache, new_lengths=[40, 1, 1, 1]))
        growth[on] = D.pool_stats()[1] - before
        assert np.isfinite(out).all() and att._cached_path == ('prefill' if on else 'fused_masked')
        assert cache.pages_in_use == 9 + 1 + 1 + 1 and cache.lengths.tolist() == [552, 4, 6, 3]
        del cache, out
    print(f'pool growth of the chunk: {growth[True]} bytes with npm_mha_prefill_fwd_f16, {growth[False]} without')
    assert growth[True] < one_gathered <= growth[False] // 2


# ---- 5. TransformerDecoder: admit a prompt among decoding sequences, fp16 caches ----------------------------------------------------------
_SLOT = (0, 1, 2, 3, 1)           # tests/test_gpu_prefill.py's plan: five logical sequences over four slots
_PLAN = [np.array(n) for n in ([44, 9, 41, 3, 0], [1, 1, 1, 1, 0], [1, 1, 1, 1, 0], [1, 0, 1, 1, 0], [1, 0, 1, 1, 40], [1, 0, 1, 1, 1],
                               [2, 0, 0, 1, 1])]
_RELEASE_AFTER, _ADMIT_AT = 2, 4


def _continuous(dec, state, q_rows, kv, kv_lengths):
    outs, paths = [], []
    for step, (x5, n5) in enumerate(VR.padded_calls(q_rows, _PLAN)):
        if step == _ADMIT_AT:
            dec.admit(state, _SLOT[4], kv[4:5], kv_length=int(kv_lengths[4]))
        x, n = np.zeros([4, x5.shape[1], x5.shape[2]], dtype=np.float32), np.zeros(4, dtype=np.int64)
        for seq in range(5):
            if n5[seq]:
                x[_SLOT[seq]], n[_SLOT[seq]] = x5[seq], n5[seq]
        out = np.asarray(dec.decode(x, state, new_lengths=n))
        assert np.isfinite(out).all(), f'step {step}: not finite'
        paths.append((dec._self_attention._cached_path, dec._cross_attention._cached_path))
        wide = np.zeros((5,) + out.shape[1:], dtype=out.dtype)
        for seq in range(5):
            if n5[seq]:
                wide[seq] = out[_SLOT[seq]]
        outs.append(wide)
        if step == _RELEASE_AFTER:
            state.release(_SLOT[1])
    return VR.collect(outs, _PLAN, 5), paths


@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('kv_heads', [None, 2])
def test_decoder_admits_a_40_token_prompt_with_f16_caches_and_PREFILL_KERNEL_F16(npm, switch, norm_first, kv_heads):
    f = 256
    dec, p = DC.make_decoder(npm, f, 4, kv_heads, 384, norm_first, True, seed=13, batch=4, seq_kv=23)
    total = VR.schedule_rows(_PLAN)
    rng = np.random.default_rng(8)
    q_rows = [rng.standard_normal([s, f]).astype(np.float32) for s in total]
    kv = rng.standard_normal([5, 40, f]).astype(np.float32)
    kv_lengths = np.array([23, 4, 11, 17, 40])
    runs = {}
    for on in (False, True):
        switch(on)
        state = dec.start_decoding(kv[:4, :23], 64, kv_lengths=kv_lengths[:4], page_size=16, pages=12, memory_capacity=48, cache_dtype='f16')
        assert state.self_cache.dtype == state.cross_cache.dtype == 'f16'
        runs[on], paths = _continuous(dec, state, q_rows, kv, kv_lengths)
        assert state.positions.tolist() == [int(total[0]), int(total[4]), int(total[2]), int(total[3])]
        assert state.self_cache.pages_in_use == sum(PC.pages_of(total[i], 16) for i in (0, 4, 2, 3))
        bulk = 'prefill' if on else 'fused_masked'
        assert paths[0] == (bulk, bulk) and paths[_ADMIT_AT] == (bulk, bulk) and paths[1] == ('decode', 'decode'), paths
    want = P16.decoder_alone_stored(p, q_rows, _PLAN, kv, kv_lengths, norm_first)
    unrounded = VR.decoder_alone(p, q_rows, _PLAN, kv, kv_lengths, norm_first)
    same = P16.decoder_alone_stored(p, q_rows, _PLAN, kv, kv_lengths, norm_first, store=lambda x: np.asarray(x, dtype=np.float64))
    assert all(np.array_equal(a, b) for a, b in zip(same, unrounded)), 'without the rounding the reference is decoder_alone'
    for i in range(5):
        alone_state = dec.start_decoding(kv[i:i + 1, :kv_lengths[i]], int(total[i]), cache_dtype='f16')   # batch 1, contiguous, switch on
        alone = np.concatenate([np.asarray(dec.decode(np.ascontiguousarray(c), alone_state))
                                for c in VR.DR_split(q_rows[i][None], [int(n[i]) for n in _PLAN])], axis=1)[0]
        print(f'admit sequence {i}: max |fp16 caches - float64 over unrounded K / V| {np.abs(runs[True][i] - unrounded[i]).max():.3e} (the storage error)')
        decode_gpu.layer_close(runs[True][i], want[i], 1e-4, f'admit sequence {i} vs float64 over K / V rounded at storage')
        decode_gpu.layer_close(runs[True][i], alone, 2 * LAYER_TOL, f'admit sequence {i} vs alone')
        decode_gpu.layer_close(runs[True][i], runs[False][i], 2 * LAYER_TOL, f'admit sequence {i} vs PREFILL_KERNEL_F16 off')
