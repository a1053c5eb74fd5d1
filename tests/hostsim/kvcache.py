"""TEST INFRASTRUCTURE ONLY -- the key / value cache and the attention over it, shaped as the product's own code is
(np_modeling_amd/csrc/npm_kvattn.h, npm_decode.hip): one row addresser for every layout and storage type (``Rows``), one argument
check (``_check_kv_attn``), one restatement of cached attention behind the eight decode / prefill entry points
(``_cached_fwd``), one of the row copies behind the four appends (``_kv_append``) and the three gathers (``_kv_gather``).
Attention is evaluated by tests/varlen_reference.py (every sequence alone, float64) or, windowed, tests/window_cases.py.

Only rows below a sequence's length, and only the table entries of their pages, are ever looked at.  What was looked at is
recorded: ``f16_reads`` (entry point, sequence, rows) of every read of an fp16 cache, ``window_reads`` (entry point, sequence,
first row, end) of every windowed sequence, ``prefix_calls`` dict(rows, prefix, splits, pages, f16) of every prefix pass,
``page_copies`` (source page, destination page, rows) and ``copy_calls`` (pairs) of every npm_kv_copy_pages and of every plane
of an npm_kv_copy_pages_planes, ``plane_calls`` (pairs, planes) of every npm_kv_copy_pages_planes, ``fused_calls``
dict(batch, tokens, rope, paged, ragged, f16) of every npm_rope_kv_append.

The two fused calls are what they fuse, made on the same unrecorded helpers as the entry points they replace (``_copy_pages``,
``Training._rope``, ``_kv_append``): each adds its own one line to ``calls``."""

import ctypes as C

import numpy as np

import decode_reference as DR
import varlen_reference as VR
import window_cases as WC

from .memory import BAD, UNSUPPORTED, _addr, _deref, _half_rows, _heads, _ints, _mat, _page_ok, _vec
from .runtime import PREFIX_MAX_SPLITS as MAX_SPLITS

HEAD_DIMS = (16, 32, 64, 128)


def auto_splits(rows, heads, kv_heads, prefix_rows):
    """npm_mha_prefix_splits with NPM_TUNE_PREFIX_SPLITS = 0."""
    if rows < 1 or heads < 1 or kv_heads < 1 or heads % kv_heads or prefix_rows < 1:
        return 1
    group = heads // kv_heads
    gb = min(group, 64)
    tiles = -(-rows // (64 // gb)) * -(-group // gb)
    return max(1, min(-(-512 // (tiles * kv_heads)), max(1, prefix_rows // 128), MAX_SPLITS))


def split_ranges(prefix_rows, splits):
    """[(first key, end)] of every split of a prefix pass: ceil(tiles / splits) tiles of 16 keys each, empty past the last tile."""
    tiles = prefix_rows // 16
    per = -(-tiles // splits)
    return [(min(s * per, tiles) * 16, min((s + 1) * per, tiles) * 16) for s in range(splits)]


class Rows:
    """The rows of a cache: row j of sequence b is row j of batch entry b (stride between entries), or with a block table row
    j % page_rows of page table[b, j // page_rows] (stride between pages).  Pitch and stride count elements, floats or halves."""

    def __init__(self, ptr, pitch, stride, row_len, table=None, table_pitch=0, page_rows=0, f16=False):
        self.ptr, self.pitch, self.stride, self.row_len = _addr(ptr), int(pitch), int(stride), int(row_len)
        self.table, self.table_pitch, self.page_rows = _addr(table), int(table_pitch), int(page_rows)
        self.view_of, self.size = (_half_rows, 2) if f16 else (_mat, 4)

    def view(self, b, j, n=1):
        """Rows j .. j + n - 1 of sequence b, all within one page, as a writable [n, row_len] view."""
        if self.table:
            page = C.c_int32.from_address(self.table + 4 * (b * self.table_pitch + j // self.page_rows)).value
            first = page * self.stride + j % self.page_rows * self.pitch
        else:
            first = b * self.stride + j * self.pitch
        return self.view_of(self.ptr + self.size * first, n, self.row_len, self.pitch)

    def runs(self, b, lo, hi):
        """(j, view of rows j ..) page by page over rows lo .. hi - 1 of sequence b."""
        while lo < hi:
            n = min(hi - lo, self.page_rows - lo % self.page_rows) if self.table else hi - lo
            yield lo, self.view(b, lo, n)
            lo += n

    def read(self, b, lo, hi, out):
        """out[lo:hi] = rows lo .. hi - 1 of sequence b: the exact conversion of what is stored."""
        for j, rows in self.runs(b, lo, hi):
            out[j:j + len(rows)] = rows.reshape((len(rows),) + out.shape[1:])


def _decode_head_ok(c):
    return c.head_dim in HEAD_DIMS and 1 <= c.heads // c.kv_heads * c.new_tokens <= 32


def _prefill_head_ok(c):
    return c.head_dim in HEAD_DIMS


def _check_kv_attn(c, lengths, block_table, table_pitch, page_rows, kv_align, head_ok):
    """check_kv_attn of np_modeling_amd/csrc/npm_kvattn.h, refusal for refusal; ``head_ok`` is the caller's own rule about
    head size and rows."""
    if c is None:
        return BAD
    if _addr(block_table):
        if not lengths or not _page_ok(page_rows) or c.kv_len < 0 or table_pitch * page_rows < c.kv_len:
            return BAD
        if c.k_stride_b < page_rows * c.k_pitch or c.v_stride_b < page_rows * c.v_pitch:
            return BAD
    if min(c.batch, c.heads, c.kv_heads, c.new_tokens, c.head_dim) < 1 or c.heads % c.kv_heads:
        return BAD
    if (c.kv_len < 0 if lengths else c.kv_len < c.new_tokens) or not c.scale > 0:
        return BAD
    if not all(_addr(p) for p in (c.q, c.k, c.v, c.ctx)):
        return BAD
    if not head_ok(c):
        return UNSUPPORTED
    if any(_addr(p) % 16 for p in (c.q, c.k, c.v, c.ctx)):
        return BAD
    if c.q_pitch % 4 or c.ctx_pitch % 4 or any(x % kv_align for x in (c.k_pitch, c.v_pitch, c.k_stride_b, c.v_stride_b)):
        return BAD
    if min(c.q_pitch, c.ctx_pitch) < c.heads * c.head_dim or min(c.k_pitch, c.v_pitch) < c.kv_heads * c.head_dim:
        return BAD
    return 0


def _check_row_copy(rows, rows_pitch, cache, pitch, stride, page_rows, batch, count, row_len, at, lens, ragged, f16):
    """row_copy of np_modeling_amd/csrc/npm_decode.hip: None for an empty call, else the code of the refusal or 0."""
    if min(batch, count, row_len, at) < 0:
        return BAD
    if batch == 0 or count == 0 or row_len == 0:
        return None
    width = 8 if f16 else 4
    if not _addr(rows) or not _addr(cache) or (ragged and not _addr(lens)) or _addr(rows) % 16 or _addr(cache) % 16:
        return BAD
    if row_len % width or rows_pitch % 4 or pitch % width or stride % width:
        return BAD
    if rows_pitch < row_len or pitch < row_len or (page_rows and stride < page_rows * pitch):
        return BAD
    return 0


class KVCache:
    def __init__(self):
        super().__init__()
        self.last_decode = self.last_prefill = self.last_prefix = self.last_rope_append = ''
        self.f16_reads, self.window_reads = [], []
        self.page_copies, self.copy_calls, self.prefix_calls = [], [], []
        self.plane_calls, self.fused_calls = [], []

    # ---- row copies -----------------------------------------------------------------------------------------------------------------
    def _kv_append(self, src, src_pitch, cache, pitch, stride, batch, tokens, row_len, at, at_lens, new_lens, ragged,
                   paged=False, table=None, table_pitch=0, page_rows=0, f16=False):
        """The append of every layout; the caller records the call.  ``ragged``: row at_lens[b] onwards of sequence b takes
        new_lens[b] rows (NULL: ``tokens``), else every sequence takes ``tokens`` rows at ``at``.  ``paged``: the cache is a page
        pool; a NULL length array or table and a bad page size are refused even when there is nothing to copy."""
        if paged and not (_addr(at_lens) and _addr(table) and table_pitch >= 0 and _page_ok(page_rows)):
            return BAD
        rc = _check_row_copy(src, src_pitch, cache, pitch, stride, page_rows if paged else 0, batch, tokens, row_len, at, at_lens,
                             ragged, f16)
        if rc != 0:
            return rc or 0
        first = _ints(at_lens, batch) if ragged else np.full(batch, at, dtype=np.int64)
        n = _ints(new_lens, batch) if ragged and _addr(new_lens) else np.full(batch, tokens, dtype=np.int64)
        new = _mat(src, batch * tokens, row_len, src_pitch)
        rows = Rows(cache, pitch, stride, row_len, table if paged else None, table_pitch, page_rows, f16)
        with np.errstate(over='ignore'):                   # a float past the halves' range is stored as inf
            for b in range(batch):
                for j, dst in rows.runs(b, int(first[b]), int(first[b] + n[b])):
                    at_src = b * tokens + j - int(first[b])
                    dst[:] = new[at_src:at_src + len(dst)].astype(dst.dtype)
        return 0

    def npm_kv_append(self, src, src_pitch, cache, cache_pitch, cache_stride_b, batch, tokens, row_len, at):
        self.calls.append('npm_kv_append')
        return self._kv_append(src, src_pitch, cache, cache_pitch, cache_stride_b, batch, tokens, row_len, at, None, None, ragged=False)

    def npm_kv_append_varlen(self, src, src_pitch, cache, cache_pitch, cache_stride_b, batch, tokens, row_len, at_lens, new_lens):
        self.calls.append('npm_kv_append_varlen')
        return self._kv_append(src, src_pitch, cache, cache_pitch, cache_stride_b, batch, tokens, row_len, 0, at_lens, new_lens,
                               ragged=True)

    def npm_kv_append_paged(self, src, src_pitch, pool, row_pitch, page_stride, batch, tokens, row_len, at_lens, new_lens,
                            block_table, table_pitch, page_rows):
        self.calls.append('npm_kv_append_paged')
        return self._kv_append(src, src_pitch, pool, row_pitch, page_stride, batch, tokens, row_len, 0, at_lens, new_lens, True, True,
                               block_table, table_pitch, page_rows)

    def npm_kv_append_f16(self, src, src_pitch, cache, cache_pitch, cache_stride, batch, tokens, row_len, at, at_lens, new_lens,
                          block_table, table_pitch, page_rows):
        self.calls.append('npm_kv_append_f16')
        paged = bool(_addr(block_table))
        return self._kv_append(src, src_pitch, cache, cache_pitch, cache_stride, batch, tokens, row_len, 0 if _addr(at_lens) else at,
                               at_lens, new_lens, paged or bool(_addr(at_lens)), paged, block_table, table_pitch, page_rows, True)

    def _kv_gather(self, entry, cache, pitch, stride, out, batch, count, row_len, lens, paged=False, table=None, table_pitch=0,
                   page_rows=0, f16=False):
        """out [batch * count, row_len] = rows 0 .. min(lens[b], count) - 1 of every sequence, zeros behind them."""
        self.calls.append(entry)
        if paged and not (_addr(lens) and _addr(table) and table_pitch >= 0 and _page_ok(page_rows)):
            return BAD
        rc = _check_row_copy(out, row_len, cache, pitch, stride, page_rows if paged else 0, batch, count, row_len, 0, lens, True, f16)
        if rc != 0:
            return rc or 0
        valid = _ints(lens, batch)
        rows = Rows(cache, pitch, stride, row_len, table if paged else None, table_pitch, page_rows, f16)
        dst = _mat(out, batch * count, row_len, row_len)
        dst[:] = 0.0
        for b in range(batch):
            take = int(min(valid[b], count))
            if take:
                if f16:
                    self.f16_reads.append(('gather', b, take))
                rows.read(b, 0, take, dst[b * count:(b + 1) * count])
        return 0

    def npm_kv_gather_varlen(self, cache, cache_pitch, cache_stride_b, out, batch, rows, row_len, lens):
        return self._kv_gather('npm_kv_gather_varlen', cache, cache_pitch, cache_stride_b, out, batch, rows, row_len, lens)

    def npm_kv_gather_paged(self, pool, row_pitch, page_stride, out, batch, rows, row_len, lens, block_table, table_pitch, page_rows):
        return self._kv_gather('npm_kv_gather_paged', pool, row_pitch, page_stride, out, batch, rows, row_len, lens, True, block_table,
                               table_pitch, page_rows)

    def npm_kv_gather_f16(self, cache, cache_pitch, cache_stride, out, batch, rows, row_len, lens, block_table, table_pitch, page_rows):
        return self._kv_gather('npm_kv_gather_f16', cache, cache_pitch, cache_stride, out, batch, rows, row_len, lens,
                               bool(_addr(block_table)), block_table, table_pitch, page_rows, True)

    def npm_kv_copy_pages(self, pool, page_stride_bytes, row_bytes, src_pages, dst_pages, rows, n):
        self.calls.append('npm_kv_copy_pages')
        return self._copy_pages(pool, page_stride_bytes, row_bytes, src_pages, dst_pages, rows, n)

    def _copy_pages(self, pool, page_stride_bytes, row_bytes, src_pages, dst_pages, rows, n):
        """The page copies of one plane; the caller records the call."""
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

    def npm_kv_copy_pages_planes(self, pool, page_stride_bytes, row_bytes, src_pages, dst_pages, rows, n, planes, plane_stride_bytes):
        """The same pairs in every plane."""
        self.calls.append('npm_kv_copy_pages_planes')
        if min(n, row_bytes, page_stride_bytes, planes, plane_stride_bytes) < 0:
            return BAD
        if n == 0 or row_bytes == 0 or planes == 0:
            return 0
        if plane_stride_bytes % 16 or (planes > 1 and plane_stride_bytes < page_stride_bytes):
            return BAD
        self.plane_calls.append((int(n), int(planes)))
        for plane in range(planes):
            rc = self._copy_pages(_addr(pool) + plane * plane_stride_bytes if _addr(pool) else None, page_stride_bytes, row_bytes,
                                  src_pages, dst_pages, rows, n)
            if rc:
                return rc
        return 0

    def npm_rope_kv_append(self, qkv, pitch, batch, tokens, heads, kv_heads, head_dim, cos, sin, table_rows, at, at_lens, new_lens,
                           k_cache, v_cache, cache_pitch, cache_stride, block_table, table_pitch, page_rows, kv_f16):
        """The three calls it fuses: the rotation of npm_rope (tests/rope_reference.py ``rotate``, the bitwise model) on the first
        heads + kv_heads heads, then the append of the layout for the k and for the v heads."""
        self.calls.append('npm_rope_kv_append')
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
            rc = self._rope(qkv, pitch, batch, tokens, heads + kv_heads, head_dim, cos, sin, table_rows, at, at_lens, 0)
            assert rc == 0
        for src, cache in parts:                    # paged implies ragged (above): one call is the append of every layout
            rc = self._kv_append(src, pitch, cache, cache_pitch, cache_stride, batch, tokens, row, 0 if ragged else at, at_lens, new_lens,
                                 ragged, paged, block_table, table_pitch, page_rows, bool(kv_f16))
            assert rc == 0
        vec = head_dim % 8 == 0 and _addr(qkv) % 16 == 0 and (not rot or (_addr(cos) % 16 == 0 and _addr(sin) % 16 == 0))
        self.last_rope_append = 'rope_kv_append_kernel D=%d vec=%d rope=%d varlen=%d paged=%d kv=%s' % (
            head_dim, vec, rot, ragged, page_rows if paged else 0, 'f16' if kv_f16 else 'f32')
        return 0

    # ---- attention over the cache ------------------------------------------------------------------------------------------------------
    def npm_mha_decode_supported(self, head_dim, group_rows):
        return int(head_dim in HEAD_DIMS and 1 <= group_rows <= 32)

    def npm_mha_prefill_supported(self, head_dim):
        return int(head_dim in HEAD_DIMS)

    npm_mha_prefix_supported = npm_mha_prefill_supported

    def npm_mha_decode_splits(self, batch, kv_heads, kv_len):
        return self.decode_splits or DR.auto_splits(batch, kv_heads, kv_len)

    def npm_mha_decode_window_splits(self, batch, kv_heads, kv_len, new_tokens, window):
        if kv_len < 1 or new_tokens < 1 or window < 1:
            return 1
        return self.npm_mha_decode_splits(batch, kv_heads, min(kv_len, window + new_tokens - 1))

    def npm_mha_prefix_splits(self, rows, heads, kv_heads, prefix_rows):
        if rows < 1 or heads < 1 or kv_heads < 1 or heads % kv_heads or prefix_rows < 1:
            return 1
        return self.prefix_splits or auto_splits(rows, heads, kv_heads, prefix_rows)

    def npm_last_decode_kernel(self):
        return self.last_decode.encode()

    def npm_last_prefill_kernel(self):
        return self.last_prefill.encode()

    def npm_last_prefix_kernel(self):
        return self.last_prefix.encode()

    def npm_last_rope_append_kernel(self):
        return self.last_rope_append.encode()

    def _cached_fwd(self, entry, dref, kv_lens=None, new_lens=None, table=None, table_pitch=0, page_rows=0, window=None, kv_f16=False):
        """Every decode / prefill entry point; ``window`` None for the plain forms.  NULL kv_lens: every sequence holds kv_len rows;
        NULL table: the contiguous cache."""
        self.calls.append(entry)
        decode = '_decode_' in entry
        c = None if dref is None else _deref(dref)
        varlen, paged = bool(_addr(kv_lens)), bool(_addr(table))
        # what the entry point refuses on its own: a NULL it does not take; a window < 1 or on a call that is not causal
        if (entry.endswith(('_varlen', '_paged', '_window')) and not varlen) or (entry.endswith('_paged') and not paged):
            return BAD
        if window is not None and (window < 1 or c is None or not c.causal):
            return BAD
        rc = _check_kv_attn(c, varlen, table, table_pitch, page_rows, 8 if kv_f16 else 4, _decode_head_ok if decode else _prefill_head_ok)
        if rc:
            return rc
        b, h, hkv, t, lmax, d = c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim
        lens = _ints(kv_lens, b) if varlen else np.full(b, lmax, dtype=np.int64)
        n = _ints(new_lens, b) if varlen and _addr(new_lens) else np.full(b, t, dtype=np.int64)
        assert (lens <= lmax).all() and (n >= 0).all() and (n <= t).all() and (not c.causal or (n <= lens).all()), (lens, n, lmax)
        first = np.zeros(b, dtype=np.int64) if window is None else WC.smallest_floor(lens, n, window)
        k, v = (np.full([b, max(int(lens.max()), 1), hkv, d], np.nan, dtype=np.float32) for _ in range(2))
        for i in range(b):
            if window is not None:
                if n[i] == 0:
                    continue
                self.window_reads.append((entry, i, int(first[i]), int(lens[i])))
            for dst, ptr, pitch, stride in ((k, c.k, c.k_pitch, c.k_stride_b), (v, c.v, c.v_pitch, c.v_stride_b)):
                if kv_f16 and window is None:
                    self.f16_reads.append(('decode' if decode else 'prefill', i, int(lens[i])))
                Rows(ptr, pitch, stride, hkv * d, table, table_pitch, page_rows, kv_f16).read(i, int(first[i]), int(lens[i]), dst[i])
        q = _heads(c.q, c.q_pitch, b, t, h, d)
        if window is None:
            ctx, lse = VR.decode_attention(q, k, v, lens, n, float(c.scale), bool(c.causal))
        else:
            ctx, lse = WC.attention(q, k, v, lens, n, float(c.scale), int(window))
        _heads(c.ctx, c.ctx_pitch, b, t, h, d)[:] = ctx
        if c.lse:
            _vec(c.lse, b * h * t)[:] = lse.ravel()
        tail = '%s%s%s%s' % (' varlen=1' if varlen else '', ' paged=%d' % page_rows if paged else '', ' kv=f16' if kv_f16 else '',
                             '' if window is None else ' window=%d' % window)
        if decode:
            if window is None:
                splits = self.npm_mha_decode_splits(b, hkv, lmax) if lmax >= 1 else 1
            else:
                splits = self.npm_mha_decode_window_splits(b, hkv, lmax, t, window)
            self.last_decode = 'mha_decode_kernel D=%d rows=%d splits=%d causal=%d%s' % (d, h // hkv * t, splits, int(bool(c.causal)), tail)
        else:
            self.last_prefill = 'mha_prefill_kernel D=%d T=%d rows=64 causal=%d%s' % (d, t, int(bool(c.causal)), tail)
        return 0

    def npm_mha_decode_fwd(self, dref):
        return self._cached_fwd('npm_mha_decode_fwd', dref)

    def npm_mha_decode_fwd_varlen(self, dref, kv_lens, new_lens):
        return self._cached_fwd('npm_mha_decode_fwd_varlen', dref, kv_lens, new_lens)

    def npm_mha_decode_fwd_paged(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows):
        return self._cached_fwd('npm_mha_decode_fwd_paged', dref, kv_lens, new_lens, block_table, table_pitch, page_rows)

    def npm_mha_decode_fwd_f16(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows):
        return self._cached_fwd('npm_mha_decode_fwd_f16', dref, kv_lens, new_lens, block_table, table_pitch, page_rows, kv_f16=True)

    def npm_mha_prefill_fwd(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows):
        return self._cached_fwd('npm_mha_prefill_fwd', dref, kv_lens, new_lens, block_table, table_pitch, page_rows)

    def npm_mha_prefill_fwd_f16(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows):
        return self._cached_fwd('npm_mha_prefill_fwd_f16', dref, kv_lens, new_lens, block_table, table_pitch, page_rows, kv_f16=True)

    def npm_mha_decode_fwd_window(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows, window, kv_f16):
        return self._cached_fwd('npm_mha_decode_fwd_window', dref, kv_lens, new_lens, block_table, table_pitch, page_rows, window, bool(kv_f16))

    def npm_mha_prefill_fwd_window(self, dref, kv_lens, new_lens, block_table, table_pitch, page_rows, window, kv_f16):
        return self._cached_fwd('npm_mha_prefill_fwd_window', dref, kv_lens, new_lens, block_table, table_pitch, page_rows, window, bool(kv_f16))

    # ---- the prefix pass ------------------------------------------------------------------------------------------------------------------
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
        if d not in HEAD_DIMS:
            return UNSUPPORTED
        align = 8 if kv_f16 else 4
        for ptr, pitch, stride in ((c.k, c.k_pitch, c.k_stride_b), (c.v, c.v_pitch, c.v_stride_b)):
            if _addr(ptr) % 16 or pitch % align or stride % align or pitch < hkv * d or stride < page_rows * pitch:
                return BAD
        if _addr(c.q) % 16 or _addr(part_ctx) % 16 or c.q_pitch % 4 or c.q_pitch < h * d:
            return BAD
        n = _ints(new_lens, b) if _addr(new_lens) else np.full(b, t, dtype=np.int64)
        pages = _ints(prefix_table, prefix_rows // page_rows)
        k, v = (np.empty([prefix_rows, hkv, d], dtype=np.float64) for _ in range(2))
        for dst, ptr, pitch, stride in ((k, c.k, c.k_pitch, c.k_stride_b), (v, c.v, c.v_pitch, c.v_stride_b)):
            # the one table row of the prefix, shared by every sequence
            Rows(ptr, pitch, stride, hkv * d, prefix_table, 0, page_rows, bool(kv_f16)).read(0, 0, prefix_rows, dst)
        assert not np.isnan(k).any() and not np.isnan(v).any(), 'a prefix page holds a row nobody wrote'
        self.prefix_calls.append(dict(rows=b * t, prefix=int(prefix_rows), splits=int(splits), pages=pages.tolist(), f16=bool(kv_f16)))
        q = _heads(c.q, c.q_pitch, b, t, h, d)
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
        if head_dim not in HEAD_DIMS:
            return UNSUPPORTED
        if _addr(part_ctx) % 16 or _addr(ctx) % 16 or ctx_pitch % 4 or ctx_pitch < heads * head_dim:
            return BAD
        n = _ints(new_lens, batch) if _addr(new_lens) else np.full(batch, tokens, dtype=np.int64)
        pc = _vec(part_ctx, splits * batch * tokens * heads * head_dim).reshape(splits, batch, tokens, heads, head_dim)
        pl = _vec(part_lse, splits * batch * tokens * heads).reshape(splits, batch, tokens, heads)
        out = _heads(ctx, ctx_pitch, batch, tokens, heads, head_dim)
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
