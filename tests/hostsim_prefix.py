"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_spec.py's simulator plus the entry points of shared key / value prefixes
(npm_kv_copy_pages, npm_mha_prefix_fwd with npm_mha_prefix_splits / npm_mha_prefix_supported / npm_last_prefix_kernel, and
npm_attn_combine), restated with NumPy in float64 with the argument checks of the entry points.

* ``page_copies`` lists (source page, destination page, rows) of every pair a npm_kv_copy_pages call carried, ``copy_calls`` the
  pair count of every call.
* ``prefix_calls`` lists dict(rows, prefix, splits, pages, f16) of every npm_mha_prefix_fwd.
* The paged attention entry points of the parent simulators read ``batch * table_pitch`` table entries whatever the lengths are;
  the real kernels read only those below ceil(length / page_rows).  A table pointer moved on behind a prefix would make the
  simulators read past the upload, so those four entry points are handed a zero-padded copy when that happens.
"""

import ctypes as C

import numpy as np

import hostsim_spec
from hostsim import _addr, _deref, _mat, _vec
from hostsim_kv16 import _half_rows
from hostsim_paged import _page_ok
from hostsim_varlen import _ints

BAD, UNSUPPORTED = 10002, 10003
MAX_SPLITS = 1024


def auto_splits(rows, heads, kv_heads, prefix_rows):
    """npm_mha_prefix_splits with NPM_TUNE_PREFIX_SPLITS = 0."""
    if rows < 1 or heads < 1 or kv_heads < 1 or heads % kv_heads or prefix_rows < 1:
        return 1
    group = heads // kv_heads
    gb = min(group, 64)
    tiles = -(-rows // (64 // gb)) * -(-group // gb)
    return max(1, min(-(-512 // (tiles * kv_heads)), max(1, prefix_rows // 128), MAX_SPLITS))


def split_ranges(prefix_rows, splits):
    """[(first key, end)] of every split: ceil(tiles / splits) tiles of 16 keys each, empty past the last tile."""
    tiles = prefix_rows // 16
    per = -(-tiles // splits)
    return [(min(s * per, tiles) * 16, min((s + 1) * per, tiles) * 16) for s in range(splits)]


class PrefixHostSim(hostsim_spec.SpecHostSim):
    prefix_splits = 0             # NPM_TUNE_PREFIX_SPLITS
    last_prefix = ''

    def __init__(self):
        super().__init__()
        self.page_copies, self.copy_calls, self.prefix_calls = [], [], []
        self._padded = None

    def npm_set_tuning(self, knob, value):
        if knob == 24:
            if not 0 <= value <= MAX_SPLITS:
                return BAD
            self.prefix_splits = int(value)
            return 0
        return super().npm_set_tuning(knob, value)

    # ---- copy-on-write ------------------------------------------------------------------------------------------------------------
    def npm_kv_copy_pages(self, pool, page_stride_bytes, row_bytes, src_pages, dst_pages, rows, n):
        self.calls.append('npm_kv_copy_pages')
        if n < 0 or row_bytes < 0 or page_stride_bytes < 0:
            return BAD
        if n == 0 or row_bytes == 0:
            return 0
        if not all(_addr(p) for p in (pool, src_pages, dst_pages, rows)):
            return BAD
        if _addr(pool) % 16 or row_bytes % 16 or page_stride_bytes % 16 or page_stride_bytes < row_bytes:
            return BAD
        src, dst, count = _ints(src_pages, n), _ints(dst_pages, n), _ints(rows, n)
        assert len(set(dst.tolist())) == n and not set(dst.tolist()) & set(src.tolist()), (src, dst)
        self.copy_calls.append(int(n))
        for s, d, r in zip(src.tolist(), dst.tolist(), count.tolist()):
            assert 0 <= r * row_bytes <= page_stride_bytes
            self.page_copies.append((s, d, r))
            C.memmove(_addr(pool) + d * page_stride_bytes, _addr(pool) + s * page_stride_bytes, r * row_bytes)
        return 0

    # ---- the prefix pass -----------------------------------------------------------------------------------------------------------
    def npm_mha_prefix_supported(self, head_dim):
        return int(head_dim in (16, 32, 64, 128))

    def npm_mha_prefix_splits(self, rows, heads, kv_heads, prefix_rows):
        if rows < 1 or heads < 1 or kv_heads < 1 or heads % kv_heads or prefix_rows < 1:
            return 1
        return self.prefix_splits or auto_splits(rows, heads, kv_heads, prefix_rows)

    def npm_last_prefix_kernel(self):
        return self.last_prefix.encode()

    def npm_mha_prefix_fwd(self, dref, new_lens, prefix_table, page_rows, prefix_rows, splits, part_ctx, part_lse, kv_f16):
        self.calls.append('npm_mha_prefix_fwd')
        if dref is None or not _addr(prefix_table) or not _page_ok(page_rows):
            return BAD
        if prefix_rows < page_rows or prefix_rows % page_rows or not 1 <= splits <= MAX_SPLITS or not _addr(part_ctx) or not _addr(part_lse):
            return BAD
        c = _deref(dref)
        b, h, hkv, t, d = c.batch, c.heads, c.kv_heads, c.new_tokens, c.head_dim
        if min(b, h, hkv, t, d) < 1 or h % hkv or not c.scale > 0 or not all(_addr(p) for p in (c.q, c.k, c.v)):
            return BAD
        if not self.npm_mha_prefix_supported(d):
            return UNSUPPORTED
        align = 8 if kv_f16 else 4
        for ptr, pitch, stride in ((c.k, c.k_pitch, c.k_stride_b), (c.v, c.v_pitch, c.v_stride_b)):
            if _addr(ptr) % 16 or pitch % align or stride % align or pitch < hkv * d or stride < page_rows * pitch:
                return BAD
        if _addr(c.q) % 16 or _addr(part_ctx) % 16 or c.q_pitch % 4 or c.q_pitch < h * d:
            return BAD
        n = _ints(new_lens, b) if _addr(new_lens) else np.full(b, t, dtype=np.int64)
        pages = _ints(prefix_table, prefix_rows // page_rows)
        size = 2 if kv_f16 else 4
        k, v = (np.concatenate([np.asarray((_half_rows if kv_f16 else _mat)(_addr(ptr) + size * int(p) * stride, page_rows, hkv * d, pitch),
                                           dtype=np.float64) for p in pages]).reshape(prefix_rows, hkv, d)
                for ptr, pitch, stride in ((c.k, c.k_pitch, c.k_stride_b), (c.v, c.v_pitch, c.v_stride_b)))
        assert not np.isnan(k).any() and not np.isnan(v).any(), 'a prefix page holds a row nobody wrote'
        self.prefix_calls.append(dict(rows=b * t, prefix=int(prefix_rows), splits=int(splits), pages=pages.tolist(), f16=bool(kv_f16)))
        q = self._heads(c.q, c.q_pitch, b, t, h, d)
        pc = _vec(part_ctx, splits * b * t * h * d).reshape(splits, b * t, h, d)
        pl = _vec(part_lse, splits * b * t * h).reshape(splits, b * t, h)
        for i in range(b):
            for tok in range(int(n[i])):
                for head in range(h):
                    x = float(c.scale) * (k[:, head % hkv] @ q[i, tok, head].astype(np.float64))
                    for s, (lo, hi) in enumerate(split_ranges(prefix_rows, splits)):
                        if hi <= lo:
                            pc[s, i * t + tok, head], pl[s, i * t + tok, head] = 0.0, -np.inf
                            continue
                        m = x[lo:hi].max()
                        p = np.exp(x[lo:hi] - m)
                        pc[s, i * t + tok, head] = (p @ v[lo:hi, head % hkv]) / p.sum()
                        pl[s, i * t + tok, head] = m + np.log(p.sum())
        self.last_prefix = 'mha_prefix_kernel D=%d R=%d rows=64 prefix=%d splits=%d paged=%d%s' % (
            d, b * t, prefix_rows, splits, page_rows, ' kv=f16' if kv_f16 else '')
        return 0

    def npm_attn_combine(self, part_ctx, part_lse, splits, ctx, ctx_pitch, lse, batch, tokens, heads, head_dim, new_lens, store_lse):
        self.calls.append('npm_attn_combine')
        if not 1 <= splits <= MAX_SPLITS or min(batch, tokens, heads) < 1 or not all(_addr(p) for p in (part_ctx, part_lse, ctx, lse)):
            return BAD
        if not self.npm_mha_prefix_supported(head_dim):
            return UNSUPPORTED
        if _addr(part_ctx) % 16 or _addr(ctx) % 16 or ctx_pitch % 4 or ctx_pitch < heads * head_dim:
            return BAD
        n = _ints(new_lens, batch) if _addr(new_lens) else np.full(batch, tokens, dtype=np.int64)
        pc = _vec(part_ctx, splits * batch * tokens * heads * head_dim).reshape(splits, batch, tokens, heads, head_dim)
        pl = _vec(part_lse, splits * batch * tokens * heads).reshape(splits, batch, tokens, heads)
        out = self._heads(ctx, ctx_pitch, batch, tokens, heads, head_dim)
        out_lse = _vec(lse, batch * heads * tokens).reshape(batch, heads, tokens)
        for i in range(batch):
            for tok in range(tokens):
                for head in range(heads):
                    if tok >= n[i]:
                        out[i, tok, head] = 0.0
                        if store_lse:
                            out_lse[i, head, tok] = -np.inf
                        continue
                    terms = [(float(pl[s, i, tok, head]), pc[s, i, tok, head]) for s in range(splits)]
                    terms.append((float(out_lse[i, head, tok]), out[i, tok, head].copy()))
                    terms = [(l, x.astype(np.float64)) for l, x in terms if l != -np.inf]
                    if not terms:
                        out[i, tok, head] = 0.0
                        continue
                    top = max(l for l, _ in terms)
                    w = np.array([np.exp(l - top) for l, _ in terms])
                    out[i, tok, head] = sum(wi * x for wi, (_, x) in zip(w, terms)) / w.sum()
                    if store_lse:
                        out_lse[i, head, tok] = top + np.log(w.sum())
        return 0

    # ---- a table pointer behind a prefix ----------------------------------------------------------------------------------------------
    def _whole_table(self, table, count):
        addr = _addr(table)
        for base, buf in self._blocks.items():
            end = buf.ctypes.data + buf.nbytes
            if base <= addr < end:
                have = (end - addr) // 4
                if have >= count:
                    return table
                self._padded = np.zeros(count, dtype=np.int32)
                self._padded[:have] = np.ctypeslib.as_array((C.c_int32 * have).from_address(addr))
                return self._padded.ctypes.data
        return table

    def npm_mha_decode_fwd_paged(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows):
        return super().npm_mha_decode_fwd_paged(dref, kv_lens, new_lens, self._whole_table(block_table, _deref(dref).batch * table_pitch),
                                                table_pitch, page_rows)

    def npm_mha_prefill_fwd(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows):
        return super().npm_mha_prefill_fwd(dref, kv_lens, new_lens, self._whole_table(block_table, _deref(dref).batch * table_pitch),
                                           table_pitch, page_rows)

    def npm_mha_decode_fwd_f16(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows):
        return super().npm_mha_decode_fwd_f16(dref, kv_lens, new_lens, self._whole_table(block_table, _deref(dref).batch * table_pitch),
                                              table_pitch, page_rows)

    def npm_mha_prefill_fwd_f16(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows):
        return super().npm_mha_prefill_fwd_f16(dref, kv_lens, new_lens, self._whole_table(block_table, _deref(dref).batch * table_pitch),
                                               table_pitch, page_rows)


def install():
    from np_modeling_amd import _C
    sim = PrefixHostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim_spec.uninstall
