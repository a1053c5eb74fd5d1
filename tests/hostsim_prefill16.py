"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_kv16.py's simulator plus the prefill attention entry point of the half-precision
cache (npm_mha_prefill_fwd_f16), restated with NumPy: the argument checks of the entry point (pitches and strides in halves,
multiples of 8; every pointer 16-byte aligned), the stored halves read back exactly through ``_read('prefill', ...)`` -- so that
``f16_reads`` shows that nothing at or past a length was looked at -- and float32 rows handed to the restatement
tests/hostsim_prefill.py uses (tests/varlen_reference.py ``decode_attention``: every sequence alone, no row limit).  ``live`` /
``peak`` count the bytes of device memory in use now / at most since a test last set ``peak = live``."""

import numpy as np

import hostsim_kv16
import varlen_reference as VR
from hostsim import _addr, _deref, _vec
from hostsim_paged import _page_ok
from hostsim_varlen import _ints


class Prefill16HostSim(hostsim_kv16.KV16HostSim):
    def __init__(self):
        super().__init__()
        self.live = self.peak = 0
        self._sizes = {}

    def npm_malloc(self, out, nbytes):
        rc = super().npm_malloc(out, nbytes)
        self._sizes[_addr(_deref(out).value)] = int(nbytes)
        self.live += int(nbytes)
        self.peak = max(self.peak, self.live)
        return rc

    def npm_free(self, ptr):
        self.live -= self._sizes.pop(_addr(ptr), 0)
        return super().npm_free(ptr)

    def npm_mha_prefill_fwd_f16(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows):
        c = _deref(dref)
        self.calls.append('npm_mha_prefill_fwd_f16')
        varlen, paged = bool(_addr(kv_lens)), bool(_addr(block_table))
        b, h, hkv, t, lmax, d = c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim
        if paged and (not varlen or not _page_ok(page_rows) or table_pitch * page_rows < lmax):
            return 10002
        if min(b, h, hkv, t, d) < 1 or h % hkv or (lmax < 0 if varlen else lmax < t) or not c.scale > 0:
            return 10002
        if not self.npm_mha_prefill_supported(d):
            return 10003
        for ptr, pitch, stride in ((c.k, c.k_pitch, c.k_stride_b), (c.v, c.v_pitch, c.v_stride_b)):
            if not self._layout_ok(ptr, pitch, stride, hkv * d, block_table, kv_lens, page_rows):
                return 10002
        if _addr(c.q) % 16 or _addr(c.ctx) % 16 or c.q_pitch % 4 or c.ctx_pitch % 4 or c.q_pitch < h * d or c.ctx_pitch < h * d:
            return 10002
        lens = _ints(kv_lens, b) if varlen else np.full(b, lmax, dtype=np.int64)
        n = _ints(new_lens, b) if varlen and _addr(new_lens) else np.full(b, t, dtype=np.int64)
        assert (lens <= lmax).all() and (n >= 0).all() and (n <= t).all() and (not c.causal or (n <= lens).all()), (lens, n, lmax)
        table = _ints(block_table, b * table_pitch).reshape(b, table_pitch) if paged else None
        rows = max(int(lens.max()), 1)
        k, v = (np.full([b, rows, hkv, d], np.nan, dtype=np.float32) for _ in range(2))
        for i in range(b):
            for dst, ptr, pitch, stride in ((k, c.k, c.k_pitch, c.k_stride_b), (v, c.v, c.v_pitch, c.v_stride_b)):
                dst[i, :lens[i]] = self._read('prefill', ptr, pitch, stride, table, page_rows, i, int(lens[i]), hkv * d).reshape(-1, hkv, d)
        q = self._heads(c.q, c.q_pitch, b, t, h, d)
        ctx, lse = VR.decode_attention(q, k, v, lens, n, float(c.scale), bool(c.causal))
        self._heads(c.ctx, c.ctx_pitch, b, t, h, d)[:] = ctx
        if c.lse:
            _vec(c.lse, b * h * t)[:] = lse.ravel()
        self.last_prefill = 'mha_prefill_kernel D=%d T=%d rows=64 causal=%d%s%s kv=f16' % (
            d, t, int(bool(c.causal)), ' varlen=1' if varlen else '', ' paged=%d' % page_rows if paged else '')
        return 0


def install():
    from np_modeling_amd import _C
    sim = Prefill16HostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim_kv16.uninstall
