"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_varlen.py's simulator plus the entry points of the paged key / value cache
(npm_mha_decode_fwd_paged, npm_kv_append_paged, npm_kv_gather_paged), restated with NumPy / tests/varlen_reference.py: the rows of
a sequence are collected through its block table and handed to the restatement of the ragged call.  Only table entries below
ceil(length / page_rows) are ever looked at.  ``uploads`` lists the byte counts of every host-to-device copy (npm_h2d is not part
of ``calls``: the existing host tests compare those lists)."""

import ctypes as C

import numpy as np

import hostsim
import hostsim_varlen
import varlen_reference as VR
from hostsim import _addr, _deref, _vec
from hostsim_varlen import _ints


def _page_ok(page_rows):
    return page_rows >= 16 and page_rows & (page_rows - 1) == 0


class PagedHostSim(hostsim_varlen.VarlenHostSim):
    def __init__(self):
        super().__init__()
        self.uploads = []

    def npm_h2d(self, dst, src, nbytes):
        self.uploads.append(int(nbytes))
        return super().npm_h2d(dst, src, nbytes)

    @staticmethod
    def _page(pool, pitch, page_stride, page, rows, row_len):
        """The first ``rows`` rows of page ``page`` as a writable [rows, row_len] view."""
        return hostsim._mat(_addr(pool) + 4 * int(page) * int(page_stride), rows, row_len, pitch)

    def _sequence(self, pool, pitch, page_stride, table_row, length, page_rows, row_len):
        """Rows 0 .. length - 1 of one sequence, contiguous [length, row_len]."""
        out = np.empty([length, row_len], dtype=np.float32)
        for first in range(0, length, page_rows):
            take = min(page_rows, length - first)
            out[first:first + take] = self._page(pool, pitch, page_stride, table_row[first // page_rows], take, row_len)
        return out

    def npm_mha_decode_fwd_paged(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows):
        c = _deref(dref)
        self.calls.append('npm_mha_decode_fwd_paged')
        if not _addr(kv_lens) or not _addr(block_table) or not _page_ok(page_rows):
            return 10002
        b, h, hkv, t, lmax, d = c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim
        if lmax < 0 or h % hkv or table_pitch * page_rows < lmax:
            return 10002
        if not self.npm_mha_decode_supported(d, h // hkv * t):
            return 10003
        lens = _ints(kv_lens, b)
        n = _ints(new_lens, b) if _addr(new_lens) else np.full(b, t, dtype=np.int64)
        assert (lens <= lmax).all() and (n >= 0).all() and (n <= t).all() and (not c.causal or (n <= lens).all()), (lens, n, lmax)
        table = _ints(block_table, b * table_pitch).reshape(b, table_pitch)
        rows = max(int(lens.max()), 1)
        k, v = (np.full([b, rows, hkv, d], np.nan, dtype=np.float32) for _ in range(2))
        for i in range(b):
            for dst, pool, pitch, stride in ((k, c.k, c.k_pitch, c.k_stride_b), (v, c.v, c.v_pitch, c.v_stride_b)):
                if pitch < hkv * d or stride < page_rows * pitch:
                    return 10002
                dst[i, :lens[i]] = self._sequence(pool, pitch, stride, table[i], int(lens[i]), page_rows, hkv * d).reshape(-1, hkv, d)
        q = self._heads(c.q, c.q_pitch, b, t, h, d)
        ctx, lse = VR.decode_attention(q, k, v, lens, n, float(c.scale), bool(c.causal))
        self._heads(c.ctx, c.ctx_pitch, b, t, h, d)[:] = ctx
        if c.lse:
            _vec(c.lse, b * h * t)[:] = lse.ravel()
        self.last_decode = 'mha_decode_kernel D=%d rows=%d splits=%d causal=%d varlen=1 paged=%d' % (
            d, h // hkv * t, self.npm_mha_decode_splits(b, hkv, lmax) if lmax >= 1 else 1, int(bool(c.causal)), page_rows)
        return 0

    def npm_kv_append_paged(self, src, src_pitch, pool, row_pitch, page_stride, batch, tokens, row_len, at_lens, new_lens,
                            block_table, table_pitch, page_rows):
        self.calls.append('npm_kv_append_paged')
        if row_len % 4 or src_pitch % 4 or row_pitch % 4 or page_stride % 4 or _addr(src) % 16 or _addr(pool) % 16 \
                or not _addr(at_lens) or not _addr(block_table) or not _page_ok(page_rows) or page_stride < page_rows * row_pitch:
            return 10002
        at = _ints(at_lens, batch)
        n = _ints(new_lens, batch) if _addr(new_lens) else np.full(batch, tokens, dtype=np.int64)
        table = _ints(block_table, batch * table_pitch).reshape(batch, table_pitch)
        rows = hostsim._mat(src, batch * tokens, row_len, src_pitch)
        for b in range(batch):
            for t in range(int(n[b])):
                j = int(at[b]) + t
                self._page(pool, row_pitch, page_stride, table[b, j // page_rows], page_rows, row_len)[j % page_rows] = rows[b * tokens + t]
        return 0

    def npm_kv_gather_paged(self, pool, row_pitch, page_stride, out, batch, rows, row_len, lens, block_table, table_pitch, page_rows):
        self.calls.append('npm_kv_gather_paged')
        if row_len % 4 or row_pitch % 4 or page_stride % 4 or _addr(pool) % 16 or _addr(out) % 16 or not _addr(lens) \
                or not _addr(block_table) or not _page_ok(page_rows) or page_stride < page_rows * row_pitch:
            return 10002
        valid = _ints(lens, batch)
        table = _ints(block_table, batch * table_pitch).reshape(batch, table_pitch)
        dst = hostsim._mat(out, batch * rows, row_len, row_len)
        dst[:] = 0.0
        for b in range(batch):
            take = int(min(valid[b], rows))
            if take:
                dst[b * rows:b * rows + take] = self._sequence(pool, row_pitch, page_stride, table[b], take, page_rows, row_len)
        return 0


def install():
    from np_modeling_amd import _C
    sim = PagedHostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim.uninstall
