"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_prefill.py's simulator plus the three entry points of the half-precision key / value
cache (npm_kv_append_f16, npm_kv_gather_f16, npm_mha_decode_fwd_f16), restated with NumPy: an append stores
``astype(np.float16)``, a gather and the attention read the stored halves back exactly and hand float32 rows to the restatement of
the ragged call (tests/varlen_reference.py).  Cache addresses are host memory holding halves; pitches and strides count halves.
``f16_reads`` lists (entry point, sequence, rows read) so that tests can see that nothing at or past a length was looked at."""

import ctypes as C

import numpy as np

import hostsim_prefill
import varlen_reference as VR
from hostsim import _addr, _deref, _mat, _vec
from hostsim_paged import _page_ok
from hostsim_varlen import _ints


def _half_rows(ptr, rows, cols, ld):
    """[rows, cols] float16 view of host memory at ``ptr`` with a row pitch of ``ld`` halves."""
    rows, cols, ld = int(rows), int(cols), int(ld)
    if rows == 0 or cols == 0:
        return np.zeros((rows, cols), dtype=np.float16)
    flat = np.ctypeslib.as_array((C.c_uint16 * ((rows - 1) * ld + cols)).from_address(_addr(ptr))).view(np.float16)
    return np.lib.stride_tricks.as_strided(flat, shape=(rows, cols), strides=(2 * ld, 2))


class KV16HostSim(hostsim_prefill.PrefillHostSim):
    def __init__(self):
        super().__init__()
        self.f16_reads = []

    @staticmethod
    def _row16(cache, pitch, stride, table, page_rows, b, j, row_len):
        """Row j of sequence b of an fp16 cache as a writable [row_len] float16 view."""
        if table is None:
            return _half_rows(_addr(cache) + 2 * (b * stride + j * pitch), 1, row_len, pitch)[0]
        return _half_rows(_addr(cache) + 2 * (int(table[b, j // page_rows]) * stride + (j % page_rows) * pitch), 1, row_len, pitch)[0]

    @staticmethod
    def _layout_ok(cache, pitch, stride, row_len, block_table, lens, page_rows):
        if _addr(cache) % 16 or pitch % 8 or stride % 8 or row_len % 8 or pitch < row_len:
            return False
        if _addr(block_table) and (not _addr(lens) or not _page_ok(page_rows) or stride < page_rows * pitch):
            return False
        return True

    def npm_kv_append_f16(self, src, src_pitch, cache, cache_pitch, cache_stride, batch, tokens, row_len, at, at_lens, new_lens,
                          block_table, table_pitch, page_rows):
        self.calls.append('npm_kv_append_f16')
        if _addr(block_table) and (not _addr(at_lens) or not _page_ok(page_rows)):
            return 10002
        if batch == 0 or tokens == 0 or row_len == 0:
            return 0
        if _addr(src) % 16 or src_pitch % 4 or src_pitch < row_len \
                or not self._layout_ok(cache, cache_pitch, cache_stride, row_len, block_table, at_lens, page_rows):
            return 10002
        first = _ints(at_lens, batch) if _addr(at_lens) else np.full(batch, at, dtype=np.int64)
        n = _ints(new_lens, batch) if _addr(at_lens) and _addr(new_lens) else np.full(batch, tokens, dtype=np.int64)
        table = _ints(block_table, batch * table_pitch).reshape(batch, table_pitch) if _addr(block_table) else None
        rows = _mat(src, batch * tokens, row_len, src_pitch)
        with np.errstate(over='ignore'):
            for b in range(batch):
                for t in range(int(n[b])):
                    self._row16(cache, cache_pitch, cache_stride, table, page_rows, b, int(first[b]) + t, row_len)[:] = \
                        rows[b * tokens + t].astype(np.float16)
        return 0

    def _read(self, what, cache, pitch, stride, table, page_rows, b, take, row_len):
        """Rows 0 .. take - 1 of sequence b as float32 [take, row_len]: the exact conversion of what is stored."""
        self.f16_reads.append((what, b, take))
        out = np.empty([take, row_len], dtype=np.float32)
        for j in range(take):
            out[j] = self._row16(cache, pitch, stride, table, page_rows, b, j, row_len)
        return out

    def npm_kv_gather_f16(self, cache, cache_pitch, cache_stride, out, batch, rows, row_len, lens, block_table, table_pitch, page_rows):
        self.calls.append('npm_kv_gather_f16')
        if _addr(block_table) and (not _addr(lens) or not _page_ok(page_rows)):
            return 10002
        if batch == 0 or rows == 0 or row_len == 0:
            return 0
        if _addr(out) % 16 or not _addr(lens) or not self._layout_ok(cache, cache_pitch, cache_stride, row_len, block_table, lens, page_rows):
            return 10002
        valid = _ints(lens, batch)
        table = _ints(block_table, batch * table_pitch).reshape(batch, table_pitch) if _addr(block_table) else None
        dst = _mat(out, batch * rows, row_len, row_len)
        dst[:] = 0.0
        for b in range(batch):
            take = int(min(valid[b], rows))
            if take:
                dst[b * rows:b * rows + take] = self._read('gather', cache, cache_pitch, cache_stride, table, page_rows, b, take, row_len)
        return 0

    def npm_mha_decode_fwd_f16(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows):
        c = _deref(dref)
        self.calls.append('npm_mha_decode_fwd_f16')
        varlen, paged = bool(_addr(kv_lens)), bool(_addr(block_table))
        b, h, hkv, t, lmax, d = c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim
        if paged and (not varlen or not _page_ok(page_rows) or table_pitch * page_rows < lmax):
            return 10002
        if min(b, h, hkv, t, d) < 1 or h % hkv or (lmax < 0 if varlen else lmax < t) or not c.scale > 0:
            return 10002
        if not self.npm_mha_decode_supported(d, h // hkv * t):
            return 10003
        for ptr, pitch, stride in ((c.k, c.k_pitch, c.k_stride_b), (c.v, c.v_pitch, c.v_stride_b)):
            if not self._layout_ok(ptr, pitch, stride, hkv * d, block_table, kv_lens, page_rows):
                return 10002
        if _addr(c.q) % 16 or _addr(c.ctx) % 16 or c.q_pitch % 4 or c.ctx_pitch % 4:
            return 10002
        lens = _ints(kv_lens, b) if varlen else np.full(b, lmax, dtype=np.int64)
        n = _ints(new_lens, b) if varlen and _addr(new_lens) else np.full(b, t, dtype=np.int64)
        assert (lens <= lmax).all() and (n >= 0).all() and (n <= t).all() and (not c.causal or (n <= lens).all()), (lens, n, lmax)
        table = _ints(block_table, b * table_pitch).reshape(b, table_pitch) if paged else None
        rows = max(int(lens.max()), 1)
        k, v = (np.full([b, rows, hkv, d], np.nan, dtype=np.float32) for _ in range(2))
        for i in range(b):
            for dst, ptr, pitch, stride in ((k, c.k, c.k_pitch, c.k_stride_b), (v, c.v, c.v_pitch, c.v_stride_b)):
                dst[i, :lens[i]] = self._read('decode', ptr, pitch, stride, table, page_rows, i, int(lens[i]), hkv * d).reshape(-1, hkv, d)
        q = self._heads(c.q, c.q_pitch, b, t, h, d)
        ctx, lse = VR.decode_attention(q, k, v, lens, n, float(c.scale), bool(c.causal))
        self._heads(c.ctx, c.ctx_pitch, b, t, h, d)[:] = ctx
        if c.lse:
            _vec(c.lse, b * h * t)[:] = lse.ravel()
        self.last_decode = 'mha_decode_kernel D=%d rows=%d splits=%d causal=%d%s%s kv=f16' % (
            d, h // hkv * t, self.npm_mha_decode_splits(b, hkv, lmax) if lmax >= 1 else 1, int(bool(c.causal)),
            ' varlen=1' if varlen else '', ' paged=%d' % page_rows if paged else '')
        return 0


def install():
    from np_modeling_amd import _C
    sim = KV16HostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim_prefill.uninstall
