"""TEST INFRASTRUCTURE ONLY -- tests/hostsim.py's host-memory simulator plus the entry points of incremental decoding
(npm_mha_decode_*, npm_kv_append, npm_last_decode_kernel) and the grouped fused forward the cached layers fall back to, restated
with NumPy / tests/decode_reference.py.  ``install()`` sets it as the product's library handle, like ``hostsim.install()``."""

import ctypes as C

import numpy as np

import decode_reference as DR
import hostsim
from hostsim import _addr, _deref, _vec


class DecodeHostSim(hostsim.HostSim):
    decode_splits = 0             # NPM_TUNE_DECODE_SPLITS
    last_decode = ''

    def npm_set_tuning(self, knob, value):
        if knob == 20:
            self.decode_splits = int(value)
        return 0

    def npm_mha_core_fwd_grouped(self, cref, kv_heads):
        """Query head h reads K / V head h % kv_heads: K / V expanded to one head per query head, then the ungrouped restatement."""
        c = _deref(cref)
        self.calls.append('npm_mha_core_fwd_grouped')
        b, h, skv, d = c.batch, c.heads, c.seq_kv, c.head_dim
        wide = []
        for ptr, pitch in ((c.k, c.k_pitch), (c.v, c.v_pitch)):
            src = self._heads(ptr, pitch, b, skv, kv_heads, d)
            wide.append(np.ascontiguousarray(src[:, :, np.arange(h) % kv_heads]))
        saved = (c.k, c.k_pitch, c.v, c.v_pitch)
        c.k, c.k_pitch, c.v, c.v_pitch = wide[0].ctypes.data, h * d, wide[1].ctypes.data, h * d
        try:
            return self.npm_mha_core_fwd(cref)
        finally:
            c.k, c.k_pitch, c.v, c.v_pitch = saved

    def npm_mha_core_bwd_grouped(self, cref, kv_heads):
        """The ungrouped restatement on expanded K / V; dK / dV of a K / V head are the sums over its query heads."""
        c = _deref(cref)
        b, h, skv, d = c.batch, c.heads, c.seq_kv, c.head_dim
        wide = [np.ascontiguousarray(self._heads(ptr, pitch, b, skv, kv_heads, d)[:, :, np.arange(h) % kv_heads])
                for ptr, pitch in ((c.k, c.k_pitch), (c.v, c.v_pitch))]
        grads = [np.zeros([b, skv, h, d], dtype=np.float32) for _ in range(2)]
        saved = (c.k, c.k_pitch, c.v, c.v_pitch, c.dk, c.dk_pitch, c.dv, c.dv_pitch)
        c.k, c.k_pitch, c.v, c.v_pitch = wide[0].ctypes.data, h * d, wide[1].ctypes.data, h * d
        c.dk, c.dk_pitch, c.dv, c.dv_pitch = grads[0].ctypes.data, h * d, grads[1].ctypes.data, h * d
        try:
            rc = self.npm_mha_core_bwd(cref)
        finally:
            c.k, c.k_pitch, c.v, c.v_pitch, c.dk, c.dk_pitch, c.dv, c.dv_pitch = saved
        for grad, ptr, pitch in ((grads[0], c.dk, c.dk_pitch), (grads[1], c.dv, c.dv_pitch)):
            self._heads(ptr, pitch, b, skv, kv_heads, d)[:] = grad.astype(np.float64).reshape(b, skv, h // kv_heads, kv_heads, d).sum(axis=2)
        return rc

    def npm_mha_decode_supported(self, head_dim, group_rows):
        return int(head_dim in (16, 32, 64, 128) and 1 <= group_rows <= 32)

    def npm_mha_decode_splits(self, batch, kv_heads, kv_len):
        return self.decode_splits or DR.auto_splits(batch, kv_heads, kv_len)

    @staticmethod
    def _cache(ptr, pitch, stride_b, b, rows, h, d):
        flat = _vec(ptr, (b - 1) * stride_b + (rows - 1) * pitch + h * d)
        return np.lib.stride_tricks.as_strided(flat, shape=(b, rows, h, d), strides=(4 * stride_b, 4 * pitch, 4 * d, 4))

    def npm_mha_decode_fwd(self, dref):
        c = _deref(dref)
        self.calls.append('npm_mha_decode_fwd')
        b, h, hkv, t, length, d = c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim
        if length < t or h % hkv:
            return 10002
        if not self.npm_mha_decode_supported(d, h // hkv * t):
            return 10003
        q = self._heads(c.q, c.q_pitch, b, t, h, d)
        k = self._cache(c.k, c.k_pitch, c.k_stride_b, b, length, hkv, d)        # rows past kv_len are never looked at
        v = self._cache(c.v, c.v_pitch, c.v_stride_b, b, length, hkv, d)
        ctx, lse = DR.decode_attention(q, k, v, length, float(c.scale), bool(c.causal))
        self._heads(c.ctx, c.ctx_pitch, b, t, h, d)[:] = ctx
        if c.lse:
            _vec(c.lse, b * h * t)[:] = lse.ravel()
        self.last_decode = 'mha_decode_kernel D=%d rows=%d splits=%d causal=%d' % (
            d, h // hkv * t, self.npm_mha_decode_splits(b, hkv, length), int(bool(c.causal)))
        return 0

    def npm_kv_append(self, src, src_pitch, cache, cache_pitch, cache_stride_b, batch, tokens, row_len, at):
        self.calls.append('npm_kv_append')
        if row_len % 4 or src_pitch % 4 or cache_pitch % 4 or cache_stride_b % 4 or _addr(src) % 16 or _addr(cache) % 16:
            return 10002
        rows = hostsim._mat(src, batch * tokens, row_len, src_pitch)
        for b in range(batch):
            hostsim._mat(_addr(cache) + 4 * (b * cache_stride_b + at * cache_pitch), tokens, row_len, cache_pitch)[:] = \
                rows[b * tokens:(b + 1) * tokens]
        return 0

    def npm_last_decode_kernel(self):
        return self.last_decode.encode()


def install():
    from np_modeling_amd import _C
    sim = DecodeHostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim.uninstall
