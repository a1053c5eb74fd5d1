"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_paged.py's simulator plus the prefill attention entry points
(npm_mha_prefill_supported, npm_mha_prefill_fwd, npm_last_prefill_kernel), restated through tests/varlen_reference.py's
``decode_attention``: the rows of every sequence are taken from the contiguous cache or collected through its block table and
each sequence is evaluated alone in float64.  No row limit; only rows below a sequence's length and table entries below
ceil(length / page_rows) are ever looked at.  ``copies`` lists the byte counts of every device-to-device copy (npm_d2d is, like
npm_h2d, not part of ``calls``: the call lists stay comparable with those of the simulators this one extends)."""

import numpy as np

import hostsim
import hostsim_paged
import varlen_reference as VR
from hostsim import _addr, _deref, _vec
from hostsim_paged import _page_ok
from hostsim_varlen import _ints


class PrefillHostSim(hostsim_paged.PagedHostSim):
    last_prefill = ''

    def __init__(self):
        super().__init__()
        self.copies = []

    def npm_d2d(self, dst, src, nbytes):
        self.copies.append(int(nbytes))
        return hostsim.HostSim.npm_h2d(self, dst, src, nbytes)

    def npm_mha_prefill_supported(self, head_dim):
        return int(head_dim in (16, 32, 64, 128))

    def npm_last_prefill_kernel(self):
        return self.last_prefill.encode()

    def npm_mha_prefill_fwd(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows):
        c = _deref(dref)
        self.calls.append('npm_mha_prefill_fwd')
        varlen, paged = bool(_addr(kv_lens)), bool(_addr(block_table))
        b, h, hkv, t, lmax, d = c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim
        if paged and (not varlen or not _page_ok(page_rows) or table_pitch * page_rows < lmax):
            return 10002
        if min(b, h, hkv, t, d) < 1 or h % hkv or (lmax < 0 if varlen else lmax < t) or not c.scale > 0:
            return 10002
        if not self.npm_mha_prefill_supported(d):
            return 10003
        lens = _ints(kv_lens, b) if varlen else np.full(b, lmax, dtype=np.int64)
        n = _ints(new_lens, b) if varlen and _addr(new_lens) else np.full(b, t, dtype=np.int64)
        assert (lens <= lmax).all() and (n >= 0).all() and (n <= t).all() and (not c.causal or (n <= lens).all()), (lens, n, lmax)
        rows = max(int(lens.max()), 1)
        if paged:
            table = _ints(block_table, b * table_pitch).reshape(b, table_pitch)
            k, v = (np.full([b, rows, hkv, d], np.nan, dtype=np.float32) for _ in range(2))
            for i in range(b):
                for dst, pool, pitch, stride in ((k, c.k, c.k_pitch, c.k_stride_b), (v, c.v, c.v_pitch, c.v_stride_b)):
                    if pitch < hkv * d or stride < page_rows * pitch:
                        return 10002
                    dst[i, :lens[i]] = self._sequence(pool, pitch, stride, table[i], int(lens[i]), page_rows, hkv * d).reshape(-1, hkv, d)
        else:
            k = self._cache(c.k, c.k_pitch, c.k_stride_b, b, rows, hkv, d)
            v = self._cache(c.v, c.v_pitch, c.v_stride_b, b, rows, hkv, d)
        q = self._heads(c.q, c.q_pitch, b, t, h, d)
        ctx, lse = VR.decode_attention(q, k, v, lens, n, float(c.scale), bool(c.causal))
        self._heads(c.ctx, c.ctx_pitch, b, t, h, d)[:] = ctx
        if c.lse:
            _vec(c.lse, b * h * t)[:] = lse.ravel()
        self.last_prefill = 'mha_prefill_kernel D=%d T=%d rows=64 causal=%d%s%s' % (
            d, t, int(bool(c.causal)), ' varlen=1' if varlen else '', ' paged=%d' % page_rows if paged else '')
        return 0


def install():
    from np_modeling_amd import _C
    sim = PrefillHostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim_paged.uninstall
