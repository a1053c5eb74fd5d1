"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_prefill16.py's simulator plus the three entry points of sliding-window attention
(npm_mha_decode_fwd_window, npm_mha_prefill_fwd_window, npm_mha_decode_window_splits), restated with NumPy: the refusals of the
entry points (window < 1, a call that is not causal, NULL kv_lens, then those of the layout and storage type), and the rows
smallest floor .. L - 1 of every sequence -- no row below, no table entry below that row's page -- read from the fp32 or fp16 cache
and handed to tests/window_cases.attention (every sequence alone, float64, the band as a mask).  ``window_reads`` lists (entry
point, sequence, first row, rows end) so that tests can see what was looked at."""

import numpy as np

import hostsim
import hostsim_prefill16
import window_cases as WC
from hostsim import _addr, _deref, _vec
from hostsim_paged import _page_ok
from hostsim_varlen import _ints


class WindowHostSim(hostsim_prefill16.Prefill16HostSim):
    def __init__(self):
        super().__init__()
        self.window_reads = []

    def npm_mha_decode_window_splits(self, batch, kv_heads, kv_len, new_tokens, window):
        if kv_len < 1 or new_tokens < 1 or window < 1:
            return 1
        return self.npm_mha_decode_splits(batch, kv_heads, min(kv_len, window + new_tokens - 1))

    def _row32(self, cache, pitch, stride, table, page_rows, b, j, row_len):
        if table is None:
            return hostsim._mat(_addr(cache) + 4 * (b * stride + j * pitch), 1, row_len, pitch)[0]
        return self._page(cache, pitch, stride, table[b, j // page_rows], page_rows, row_len)[j % page_rows]

    def _window_fwd(self, entry, dref, kv_lens, new_lens, block_table, table_pitch, page_rows, window, kv_f16):
        self.calls.append(entry)
        if window < 1 or dref is None:
            return 10002
        c = _deref(dref)
        if not c.causal or not _addr(kv_lens):
            return 10002
        paged = bool(_addr(block_table))
        b, h, hkv, t, lmax, d = c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim
        if paged and (not _page_ok(page_rows) or table_pitch * page_rows < lmax):
            return 10002
        if min(b, h, hkv, t, d) < 1 or h % hkv or lmax < 0 or not c.scale > 0:
            return 10002
        decode = entry == 'npm_mha_decode_fwd_window'
        if not (self.npm_mha_decode_supported(d, h // hkv * t) if decode else self.npm_mha_prefill_supported(d)):
            return 10003
        align = 8 if kv_f16 else 4
        for ptr, pitch, stride in ((c.k, c.k_pitch, c.k_stride_b), (c.v, c.v_pitch, c.v_stride_b)):
            if _addr(ptr) % 16 or pitch % align or stride % align or pitch < hkv * d or (paged and stride < page_rows * pitch):
                return 10002
        if _addr(c.q) % 16 or _addr(c.ctx) % 16 or c.q_pitch % 4 or c.ctx_pitch % 4 or c.q_pitch < h * d or c.ctx_pitch < h * d:
            return 10002
        lens = _ints(kv_lens, b)
        n = _ints(new_lens, b) if _addr(new_lens) else np.full(b, t, dtype=np.int64)
        assert (lens <= lmax).all() and (n >= 0).all() and (n <= t).all() and (n <= lens).all(), (lens, n, lmax)
        table = _ints(block_table, b * table_pitch).reshape(b, table_pitch) if paged else None
        first = WC.smallest_floor(lens, n, window)
        rows = max(int(lens.max()), 1)
        k, v = (np.full([b, rows, hkv, d], np.nan, dtype=np.float32) for _ in range(2))
        row = self._row16 if kv_f16 else self._row32
        for i in range(b):
            if n[i] == 0:
                continue
            self.window_reads.append((entry, i, int(first[i]), int(lens[i])))
            for dst, ptr, pitch, stride in ((k, c.k, c.k_pitch, c.k_stride_b), (v, c.v, c.v_pitch, c.v_stride_b)):
                for j in range(int(first[i]), int(lens[i])):
                    dst[i, j] = np.asarray(row(ptr, pitch, stride, table, page_rows, i, j, hkv * d), dtype=np.float32).reshape(hkv, d)
        q = self._heads(c.q, c.q_pitch, b, t, h, d)
        ctx, lse = WC.attention(q, k, v, lens, n, float(c.scale), int(window))
        self._heads(c.ctx, c.ctx_pitch, b, t, h, d)[:] = ctx
        if c.lse:
            _vec(c.lse, b * h * t)[:] = lse.ravel()
        tail = ' varlen=1%s%s window=%d' % (' paged=%d' % page_rows if paged else '', ' kv=f16' if kv_f16 else '', window)
        if decode:
            splits = self.npm_mha_decode_window_splits(b, hkv, lmax, t, window)
            self.last_decode = 'mha_decode_kernel D=%d rows=%d splits=%d causal=1%s' % (d, h // hkv * t, splits, tail)
        else:
            self.last_prefill = 'mha_prefill_kernel D=%d T=%d rows=64 causal=1%s' % (d, t, tail)
        return 0

    def npm_mha_decode_fwd_window(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows, window, kv_f16):
        return self._window_fwd('npm_mha_decode_fwd_window', dref, kv_lens, new_lens, block_table, table_pitch, page_rows, window, kv_f16)

    def npm_mha_prefill_fwd_window(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows, window, kv_f16):
        return self._window_fwd('npm_mha_prefill_fwd_window', dref, kv_lens, new_lens, block_table, table_pitch, page_rows, window, kv_f16)


def install():
    from np_modeling_amd import _C
    sim = WindowHostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim_prefill16.uninstall
