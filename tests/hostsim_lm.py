"""TEST INFRASTRUCTURE ONLY -- the host simulator plus what a decoder-only language model calls beyond it, by composition.

``LmLib`` wraps the simulator the way tests/hostsim_llama.py's ``LlamaLib`` does -- it IS a ``LlamaLib`` (npm_rmsnorm_*,
npm_swiglu_*) around an ``XentLib`` (npm_softmax_xent_rows) around the simulator -- and restates npm_kv_copy_pages_planes from the
simulator's own npm_kv_copy_pages -- the same pairs in every plane; ``plane_calls`` lists (pairs, planes) of every call -- and
npm_rope_kv_append from the simulator's npm_rope (tests/rope_reference.py) and its own appends (``fused_calls``).
``install()`` puts it where the product looks for its library."""

from hostsim import install as install_sim
from hostsim.kvcache import _check_row_copy
from hostsim.memory import BAD, _addr, _page_ok
from hostsim_llama import LlamaLib
from hostsim_xent import XentLib


class LmLib(LlamaLib):
    def __init__(self, sim):
        self.raw = sim
        self.plane_calls, self.fused_calls, self._last_fused = [], [], b''
        LlamaLib.__init__(self, XentLib(sim))

    def npm_kv_copy_pages_planes(self, pool, page_stride_bytes, row_bytes, src_pages, dst_pages, rows, n, planes, plane_stride_bytes):
        sim = self.raw
        sim.calls.append('npm_kv_copy_pages_planes')
        if min(n, row_bytes, page_stride_bytes, planes, plane_stride_bytes) < 0:
            return BAD
        if n == 0 or row_bytes == 0 or planes == 0:
            return 0
        if plane_stride_bytes % 16 or (planes > 1 and plane_stride_bytes < page_stride_bytes):
            return BAD
        self.plane_calls.append((int(n), int(planes)))
        for plane in range(planes):
            rc = sim.npm_kv_copy_pages(_addr(pool) + plane * plane_stride_bytes if _addr(pool) else None, page_stride_bytes, row_bytes,
                                       src_pages, dst_pages, rows, n)
            assert sim.calls.pop() == 'npm_kv_copy_pages'          # the restatement's own use of it is not a call of the product
            if rc:
                return rc
        return 0

    def npm_rope_kv_append(self, qkv, pitch, batch, tokens, heads, kv_heads, head_dim, cos, sin, table_rows, at, at_lens, new_lens,
                           k_cache, v_cache, cache_pitch, cache_stride, block_table, table_pitch, page_rows, kv_f16):
        """The three calls it fuses, made on the simulator: its npm_rope (tests/rope_reference.py ``rotate``, the bitwise model)
        on the first heads + kv_heads heads, then its own append of the layout for the k and for the v heads."""
        sim = self.raw
        sim.calls.append('npm_rope_kv_append')
        rot, paged, ragged = bool(_addr(cos) or _addr(sin)), bool(_addr(block_table)), bool(_addr(at_lens))
        self.fused_calls.append(dict(batch=batch, tokens=tokens, rope=rot, paged=paged, ragged=ragged, f16=bool(kv_f16)))
        if paged and not (ragged and table_pitch >= 0 and _page_ok(page_rows)):
            return BAD
        if min(heads, kv_heads, head_dim) < 1:
            return BAD
        # every refusal first, as the kernel's host function has it: a refused call writes nothing
        if rot:
            if not (_addr(qkv) and _addr(cos) and _addr(sin)) or min(batch, tokens, table_rows) < 1 or head_dim < 2 or head_dim % 2:
                return BAD
            if not ragged and (at < 0 or at + tokens > table_rows):
                return BAD
        if min(batch, tokens) < 0 or (not ragged and at < 0):
            return BAD
        if batch == 0 or tokens == 0:
            return 0
        if head_dim % 2 or pitch < (heads + 2 * kv_heads) * head_dim or not _addr(qkv):
            return BAD
        row = kv_heads * head_dim
        parts = ((_addr(qkv) + 4 * heads * head_dim, k_cache), (_addr(qkv) + 4 * (heads * head_dim + row), v_cache))
        for src, cache in parts:
            rc = _check_row_copy(src, pitch, cache, cache_pitch, cache_stride, page_rows if paged else 0, batch, tokens, row,
                                 0 if ragged else at, at_lens, ragged, bool(kv_f16))
            if rc:
                return rc
        if rot:
            rc = sim.npm_rope(qkv, pitch, batch, tokens, heads + kv_heads, head_dim, cos, sin, table_rows, at, at_lens, 0)
            assert rc == 0 and sim.calls.pop() == 'npm_rope'     # the restatement's own use of it is not a call of the product
            sim.ropes.pop()
        for src, cache in parts:
            if kv_f16:
                rc = sim.npm_kv_append_f16(src, pitch, cache, cache_pitch, cache_stride, batch, tokens, row, at, at_lens, new_lens,
                                           block_table, table_pitch, page_rows)
            elif paged:
                rc = sim.npm_kv_append_paged(src, pitch, cache, cache_pitch, cache_stride, batch, tokens, row, at_lens, new_lens,
                                             block_table, table_pitch, page_rows)
            elif ragged:
                rc = sim.npm_kv_append_varlen(src, pitch, cache, cache_pitch, cache_stride, batch, tokens, row, at_lens, new_lens)
            else:
                rc = sim.npm_kv_append(src, pitch, cache, cache_pitch, cache_stride, batch, tokens, row, at)
            assert rc == 0 and sim.calls.pop().startswith('npm_kv_append')
        vec = head_dim % 8 == 0 and _addr(qkv) % 16 == 0 and (not rot or (_addr(cos) % 16 == 0 and _addr(sin) % 16 == 0))
        self._last_fused = ('rope_kv_append_kernel D=%d vec=%d rope=%d varlen=%d paged=%d kv=%s' % (
            head_dim, vec, rot, ragged, page_rows if paged else 0, 'f16' if kv_f16 else 'f32')).encode()
        return 0

    def npm_last_rope_append_kernel(self):
        return self._last_fused


def install(profile=None):
    """A fresh simulator wrapped in an ``LmLib``, installed as the product's library handle; returns the wrapper."""
    from np_modeling_amd import _C
    lib = LmLib(install_sim(profile))
    _C._LIB = lib
    return lib
