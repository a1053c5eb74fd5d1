"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_decode.py's simulator plus the entry points of ragged batches
(npm_mha_decode_fwd_varlen, npm_kv_append_varlen, npm_kv_gather_varlen), restated with NumPy / tests/varlen_reference.py.  The
length arrays are "device" int32: addresses of host memory, as every pointer of the simulator."""

import ctypes as C

import numpy as np

import hostsim
import hostsim_decode
import varlen_reference as VR
from hostsim import _addr, _deref, _vec


def _ints(ptr, n):
    return np.ctypeslib.as_array((C.c_int32 * int(n)).from_address(_addr(ptr))).astype(np.int64)


class VarlenHostSim(hostsim_decode.DecodeHostSim):
    def npm_mha_decode_fwd_varlen(self, dref, kv_lens, new_lens):
        c = _deref(dref)
        self.calls.append('npm_mha_decode_fwd_varlen')
        if not _addr(kv_lens):
            return 10002
        b, h, hkv, t, lmax, d = c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim
        if lmax < 0 or h % hkv:
            return 10002
        if not self.npm_mha_decode_supported(d, h // hkv * t):
            return 10003
        lens = _ints(kv_lens, b)
        n = _ints(new_lens, b) if _addr(new_lens) else np.full(b, t, dtype=np.int64)
        assert (lens <= lmax).all() and (n >= 0).all() and (n <= t).all() and (not c.causal or (n <= lens).all()), (lens, n, lmax)
        q = self._heads(c.q, c.q_pitch, b, t, h, d)
        rows = max(int(lens.max()), 1)                                            # nothing at or past a sequence's length is looked at
        k = self._cache(c.k, c.k_pitch, c.k_stride_b, b, rows, hkv, d)
        v = self._cache(c.v, c.v_pitch, c.v_stride_b, b, rows, hkv, d)
        ctx, lse = VR.decode_attention(q, k, v, lens, n, float(c.scale), bool(c.causal))
        self._heads(c.ctx, c.ctx_pitch, b, t, h, d)[:] = ctx
        if c.lse:
            _vec(c.lse, b * h * t)[:] = lse.ravel()
        self.last_decode = 'mha_decode_kernel D=%d rows=%d splits=%d causal=%d varlen=1' % (
            d, h // hkv * t, self.npm_mha_decode_splits(b, hkv, lmax) if lmax >= 1 else 1, int(bool(c.causal)))
        return 0

    def npm_kv_append_varlen(self, src, src_pitch, cache, cache_pitch, cache_stride_b, batch, tokens, row_len, at_lens, new_lens):
        self.calls.append('npm_kv_append_varlen')
        if row_len % 4 or src_pitch % 4 or cache_pitch % 4 or cache_stride_b % 4 or _addr(src) % 16 or _addr(cache) % 16 \
                or not _addr(at_lens):
            return 10002
        at = _ints(at_lens, batch)
        n = _ints(new_lens, batch) if _addr(new_lens) else np.full(batch, tokens, dtype=np.int64)
        rows = hostsim._mat(src, batch * tokens, row_len, src_pitch)
        for b in range(batch):
            if n[b]:
                hostsim._mat(_addr(cache) + 4 * (b * cache_stride_b + int(at[b]) * cache_pitch), int(n[b]), row_len, cache_pitch)[:] = \
                    rows[b * tokens:b * tokens + int(n[b])]
        return 0

    def npm_kv_gather_varlen(self, cache, cache_pitch, cache_stride_b, out, batch, rows, row_len, lens):
        self.calls.append('npm_kv_gather_varlen')
        if row_len % 4 or cache_pitch % 4 or cache_stride_b % 4 or _addr(cache) % 16 or _addr(out) % 16 or not _addr(lens):
            return 10002
        valid = _ints(lens, batch)
        dst = hostsim._mat(out, batch * rows, row_len, row_len)
        dst[:] = 0.0
        for b in range(batch):
            take = int(min(valid[b], rows))
            if take:
                dst[b * rows:b * rows + take] = hostsim._mat(_addr(cache) + 4 * b * cache_stride_b, take, row_len, cache_pitch)
        return 0


def install():
    from np_modeling_amd import _C
    sim = VarlenHostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim.uninstall
