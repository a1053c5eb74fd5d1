#!/usr/bin/env python3
"""What a sliding window saves the decode attention (npm_mha_decode_fwd_window, csrc/npm_decode.hip) at T = 1 new token, Hq 8,
D 128, B 64, page 64, Hkv in {8, 1}, with the method of tools/decode_paged_bench.py: time per call from HIP events around a window
of back-to-back calls (the combine launch included), min / median / max over the windows, "cold" K / V.

Three things, same pools, same process, interleaved:

  (a) npm_mha_decode_fwd_paged at L = Lmax (8192)                     what a step costs without a window
  (w) npm_mha_decode_fwd_window at L = Lmax, W in {512, 1024, 4096}   the windowed step
  (y) npm_mha_decode_fwd_paged at L = W                               the YARDSTICK: what a window of W should cost

Cold K / V: a pool is a slice [B, Lmax, Hkv, D] of an arena, B Lmax / page pages.  The block table of call i maps the logical
pages a call reads -- the last W rows of every sequence for (w), the first W rows for (y) -- onto the physical pages of region
i mod (Lmax / W) of the sequence's part of the slice, so consecutive calls read different memory and a sweep covers the whole
slice (larger than the 256 MB Infinity Cache for every row of the table below; Hkv 1 also rotates over the slices of its arena).
(w) and (y) thus read the same physical pages in the same order; what differs is the entry point, L and the position of the rows
in the sequence.

Then the pages a PagedKVCache holds after decoding to Lmax with and without the window (real appends; host accounting).

    python tools/decode_window_bench.py > profiles/r17_decode_window_bench.log
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARENA_BYTES = 1 << 30


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--b', type=int, default=64)
    ap.add_argument('--lmax', type=int, default=8192)
    ap.add_argument('--kv', default='8,1')
    ap.add_argument('--h', type=int, default=8)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--page', type=int, default=64)
    ap.add_argument('--w', default='512,1024,4096', help='windows')
    ap.add_argument('--windows', type=int, default=7, help='timing windows per row')
    ap.add_argument('--window-ms', type=float, default=8.0)
    ap.add_argument('--no-pages', action='store_true', help='skip the pages-in-use part')
    a = ap.parse_args()

    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    b, lmax, h, d, page = a.b, a.lmax, a.h, a.d, a.page
    wins = [int(x) for x in a.w.split(',')]
    assert lmax % page == 0 and all(w % page == 0 and lmax % w == 0 for w in wins), 'Lmax and every W: multiples of the page, W | Lmax'
    per = lmax // page
    scale = 1.0 / np.sqrt(d)
    print(f'decode_window_bench: sources {_C.source_id()}, B {b} Lmax {lmax} Hq {h} D {d} T 1 page {page}; {a.windows} windows of '
          f'~{a.window_ms} ms after one untimed window; microseconds per call', flush=True)

    def window(fn, calls):
        start = D.Event().record()
        for i in range(calls):
            fn(i)
        stop = D.Event().record()
        stop.synchronize()
        return start.elapsed_ms(stop) * 1e3 / calls

    def measure(fn):
        calls = 8
        window(fn, calls)
        us = window(fn, calls)
        calls = int(max(8, min(4000, a.window_ms * 1e3 / max(us, 1.0))))
        window(fn, calls)
        t = sorted(window(fn, calls) for _ in range(a.windows))
        return t[0], t[len(t) // 2], t[-1]

    for hkv in (int(x) for x in a.kv.split(',')):
        floats = b * lmax * hkv * d
        arena = max(ARENA_BYTES // 4, floats)
        slots = max(1, arena // floats)
        ka, va = D.full([arena], 0.01), D.full([arena], 0.02)
        q = D.from_host(np.random.default_rng(0).standard_normal([b, 1, h, d]).astype(np.float32))
        ctx, lse = D.empty([b, 1, h, d]), D.empty([b, h, 1])
        dec = _C.npm_mha_decode()
        dec.batch, dec.heads, dec.kv_heads, dec.new_tokens, dec.head_dim = b, h, hkv, 1, d
        dec.causal, dec.scale = 1, scale
        dec.q, dec.q_pitch, dec.ctx, dec.ctx_pitch, dec.lse = q.ptr, h * d, ctx.ptr, h * d, lse.ptr
        dec.k_pitch = dec.v_pitch = hkv * d
        dec.k_stride_b = dec.v_stride_b = page * hkv * d
        ones = D.bytes_from_host(np.ones(b, dtype=np.int32))

        def tables(first_page, pages_read):
            """One table per region: logical pages first_page .. first_page + pages_read - 1 of sequence b land on the physical
            pages of region r of that sequence's part of the slice; the other entries stay inside it too (they are not read)."""
            out = []
            for r in range(per // pages_read):
                shift = (r * pages_read - first_page) % per
                t = (np.arange(b, dtype=np.int64)[:, None] * per + (np.arange(per)[None, :] + shift) % per).astype(np.int32)
                out.append(D.bytes_from_host(np.ascontiguousarray(t)))
            return out

        def paged(length, tabs):
            lens = D.bytes_from_host(np.full(b, length, dtype=np.int32))

            def run(i):
                off = 4 * floats * (i % slots)
                dec.k, dec.v, dec.kv_len = ka.ptr + off, va.ptr + off, length
                tab = tabs[(i // slots) % len(tabs)]
                _C.check(lib.npm_mha_decode_fwd_paged(C.byref(dec), lens.ptr, ones.ptr, tab.ptr, per, page), 'npm_mha_decode_fwd_paged')
            return run

        def windowed(w, tabs):
            lens = D.bytes_from_host(np.full(b, lmax, dtype=np.int32))

            def run(i):
                off = 4 * floats * (i % slots)
                dec.k, dec.v, dec.kv_len = ka.ptr + off, va.ptr + off, lmax
                tab = tabs[(i // slots) % len(tabs)]
                _C.check(lib.npm_mha_decode_fwd_window(C.byref(dec), lens.ptr, ones.ptr, tab.ptr, per, page, w, 0), 'npm_mha_decode_fwd_window')
            return run

        def row(tag, t, extra=''):
            print(f'Hkv {hkv} {tag:<44} {t[0]:8.1f} {t[1]:8.1f} {t[2]:8.1f}{extra}', flush=True)

        print(f'Hkv {hkv}: {slots} K / V slice(s) of {8.0 * floats / 2 ** 20:.0f} MB; splits {lib.npm_mha_decode_splits(b, hkv, lmax)} at L {lmax}'
              f'{"":>14} min      med      max', flush=True)
        ta = measure(paged(lmax, tables(0, per)))
        row(f'(a) unwindowed paged, L {lmax}', ta, f'   spread {(ta[2] - ta[0]) / ta[1]:.1%}')
        for w in wins:
            last, first = tables(per - w // page, w // page), tables(0, w // page)
            ty = measure(paged(w, first))
            tw = measure(windowed(w, last))
            ty2 = measure(paged(w, first))
            med = 0.5 * (ty[1] + ty2[1])
            row(f'(y) unwindowed paged, L = W = {w}', ty, f'   splits {lib.npm_mha_decode_splits(b, hkv, w)}')
            row(f'(w) windowed, L {lmax}, W {w}', tw, f'   / (y) {tw[1] / med:.3f}   / (a) {tw[1] / ta[1]:.3f}   splits '
                f'{lib.npm_mha_decode_window_splits(b, hkv, lmax, 1, w)}')
            row(f'(y) again, L = W = {w}', ty2, f'   (y) moved {ty2[1] / ty[1]:.3f}')
        ta2 = measure(paged(lmax, tables(0, per)))
        row(f'(a) again, L {lmax}', ta2, f'   (a) moved {ta2[1] / ta[1]:.3f}')
        del ka, va
        D.trim_pool()

    if a.no_pages:
        return
    print(f'pages of {page} rows a PagedKVCache holds after decoding B {b} sequences to {lmax} tokens (chunks of {page}, then single tokens), '
          f'and the MB of K + V in them:')
    for hkv in (int(x) for x in a.kv.split(',')):
        row_len = hkv * d
        chunk = D.zeros([b, page, row_len])
        for w in [None] + wins:
            pool = None if w is None else b * (-(-(w - 1 + page) // page) + 1)
            cache = D.PagedKVCache(b, lmax, hkv, d, page_size=page, pages=pool, window=w)
            most = 0
            while cache.max_length < lmax:
                t = page if cache.max_length + page < lmax else 1
                cache.append(D.Mat(chunk, row_len), D.Mat(chunk, row_len), t)
                most = max(most, cache.pages_in_use)
            mb = 2 * 4 * page * row_len / 2 ** 20
            print(f'Hkv {hkv} window {str(w):>5}: pages in use {cache.pages_in_use:6d} (most {most:6d}, pool {cache.pages:6d})   '
                  f'{cache.pages_in_use * mb:8.1f} MB in use, pool {cache.pages * mb:8.1f} MB', flush=True)
            del cache
            D.trim_pool()


if __name__ == '__main__':
    main()
