#!/usr/bin/env python3
"""What reading K / V through a block table costs the decode attention (npm_mha_decode_fwd_paged, csrc/npm_decode.hip) at T = 1
new token, Hq 8, D 128, B 64, Lmax 8192, Hkv in {8, 1}, with the method of tools/decode_ragged_bench.py: time per call from HIP
events around a window of back-to-back calls (the combine launch included), min / median / max over the windows; "cold" K / V
(every call of a window reads a different slice of two arenas far larger than the 256 MB Infinity Cache; a K / V pair larger than
that is its own arena).

A slice is laid out [B, Lmax, Hkv, D] and is ALSO a pool of B Lmax / page_rows pages (page stride page_rows Hkv D): under the
identity table sequence b owns pages b P .. b P + P - 1 and the paged call reads the very addresses the contiguous call reads;
under the random table the pages of the slice are dealt out in a seeded random order.  Same contents, same process, interleaved:

  (a) npm_mha_decode_fwd_varlen on the contiguous slice                   the baseline, measured before and after the paged rows
  (b) npm_mha_decode_fwd_paged, identity table                            the table lookup alone
  (c) npm_mha_decode_fwd_paged, pages in a seeded random order            the lookup and the scattered pages

for page sizes 16, 64 and 256, at all lengths = Lmax and at the two ragged draws of tools/decode_ragged_bench.py (lengths uniform
in 1 .. Lmax, seeded; one sequence at Lmax and the others at Lmax / 16), with the ratios of the medians to (a)'s and whether a
row lies inside (a)'s own min .. max over both of its measurements; then npm_mha_decode_fwd at Lmax beside the number
profiles/r09_decode_ragged_bench.log holds for it; then the bytes of HBM a contiguous cache and a paged cache hold for each draw.

    python tools/decode_paged_bench.py > profiles/r10_decode_paged_bench.log
    rocprofv3 --kernel-trace --stats -d DIR -o paged -- python tools/decode_paged_bench.py --kv 8 --only skewed --pages 16
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARENA_BYTES = 1 << 30
# profiles/r09_decode_ragged_bench.log, B 64 Lmax 8192, medians of its two runs: npm_mha_decode_fwd at Lmax, varlen at all lengths Lmax
R09 = {8: ((698.9, 637.7), (700.3, 638.1)), 1: ((97.7, 97.2), (96.0, 97.7))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--b', type=int, default=64)
    ap.add_argument('--lmax', type=int, default=8192)
    ap.add_argument('--kv', default='8,1')
    ap.add_argument('--h', type=int, default=8)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--pages', default='16,64,256', help='page sizes')
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=8.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--only', default='', help='one draw only (full, uniform, skewed): for a profiler run')
    a = ap.parse_args()

    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    b, lmax, h, d = a.b, a.lmax, a.h, a.d
    sizes = [int(x) for x in a.pages.split(',')]
    assert all(lmax % s == 0 for s in sizes), 'Lmax must be a multiple of every page size (a slice doubles as a pool)'
    scale = 1.0 / np.sqrt(d)
    print(f'decode_paged_bench: sources {_C.source_id()}, B {b} Lmax {lmax} Hq {h} D {d} T 1; {a.windows} windows of ~{a.window_ms} ms '
          f'after one untimed window; microseconds per call', flush=True)

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

    rng = np.random.default_rng(a.seed)
    draws = {'full': np.full(b, lmax), 'uniform': rng.integers(1, lmax + 1, b), 'skewed': np.array([lmax] + [lmax // 16] * (b - 1))}
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

        def uniform(i):
            off = 4 * floats * (i % slots)
            dec.k, dec.v, dec.kv_len = ka.ptr + off, va.ptr + off, lmax
            dec.k_stride_b = dec.v_stride_b = lmax * hkv * d
            _C.check(lib.npm_mha_decode_fwd(C.byref(dec)), 'npm_mha_decode_fwd')

        def varlen(lengths):
            dev = D.bytes_from_host(np.ascontiguousarray(np.asarray(lengths, dtype=np.int32)))

            def run(i, dev=dev):
                off = 4 * floats * (i % slots)
                dec.k, dec.v, dec.kv_len = ka.ptr + off, va.ptr + off, lmax
                dec.k_stride_b = dec.v_stride_b = lmax * hkv * d
                _C.check(lib.npm_mha_decode_fwd_varlen(C.byref(dec), dev.ptr, None), 'npm_mha_decode_fwd_varlen')
            return run

        def paged(lengths, page_rows, order):
            per = lmax // page_rows
            table = np.arange(b * per, dtype=np.int32)
            if order == 'random':
                table = np.random.default_rng(a.seed + page_rows).permutation(b * per).astype(np.int32)
            dev = D.bytes_from_host(np.ascontiguousarray(np.asarray(lengths, dtype=np.int32)))
            tab = D.bytes_from_host(np.ascontiguousarray(table))

            def run(i, dev=dev, tab=tab):
                off = 4 * floats * (i % slots)
                dec.k, dec.v, dec.kv_len = ka.ptr + off, va.ptr + off, lmax
                dec.k_stride_b = dec.v_stride_b = page_rows * hkv * d
                _C.check(lib.npm_mha_decode_fwd_paged(C.byref(dec), dev.ptr, None, tab.ptr, per, page_rows), 'npm_mha_decode_fwd_paged')
            return run

        def row(tag, t, extra=''):
            print(f'Hkv {hkv} {tag:<48} {t[0]:8.1f} {t[1]:8.1f} {t[2]:8.1f}{extra}', flush=True)

        splits = lib.npm_mha_decode_splits(b, hkv, lmax)
        print(f'Hkv {hkv}: splits {splits} (of Lmax), {slots} K / V slice(s) of {8.0 * floats / 2 ** 20:.0f} MB;'
              f'{"":>26} min      med      max', flush=True)
        for name, lengths in draws.items():
            if a.only not in ('', name):
                continue
            total = int(lengths.sum())
            what = f'{name}: sum {total} = {total / (b * lmax):.3f} B Lmax'
            ta = measure(varlen(lengths))
            row(f'(a) varlen contiguous, {what}', ta, f'   spread {(ta[2] - ta[0]) / ta[1]:.1%}')
            rows = []
            for page_rows in sizes:
                for tag, order in (('(b) paged identity', 'identity'), ('(c) paged random', 'random')):
                    rows.append((f'{tag} page {page_rows}, {name}', measure(paged(lengths, page_rows, order))))
            ta2 = measure(varlen(lengths))
            lo, hi, med = min(ta[0], ta2[0]), max(ta[2], ta2[2]), 0.5 * (ta[1] + ta2[1])
            for tag, t in rows:
                where = 'below' if t[1] < lo else 'inside' if t[1] <= hi else 'above, inside + 3 % of' if t[1] <= hi * 1.03 else 'OUTSIDE + 3 % of'
                row(tag, t, f'   / (a) {t[1] / med:.3f}   median {where} (a) min .. max {lo:.1f} .. {hi:.1f}')
            row(f'(a) again, {name}', ta2, f'   (a) moved {ta2[1] / ta[1]:.3f}')
        if not a.only:
            tu = measure(uniform)
            ref = R09.get(hkv) if (b, lmax, h, d) == (64, 8192, 8, 128) else None
            row(f'npm_mha_decode_fwd L = {lmax}', tu, f'   r09 log medians: decode_fwd {ref[0][0]:.1f} / {ref[0][1]:.1f}, varlen full '
                f'{ref[1][0]:.1f} / {ref[1][1]:.1f}' if ref else '')
        del ka, va
        D.trim_pool()

    print('HBM held by K + V of one attention layer (MB), contiguous [B, Lmax, Hkv, D] against the pages in use:')
    for hkv in (int(x) for x in a.kv.split(',')):
        row_bytes = 2 * 4 * hkv * d
        for name, lengths in draws.items():
            held = ', '.join(f'page {s}: {int(np.sum(-(-lengths // s)) * s) * row_bytes / 2 ** 20:.1f}' for s in sizes)
            print(f'Hkv {hkv} {name:<8} contiguous {b * lmax * row_bytes / 2 ** 20:.1f}   keys {int(lengths.sum()) * row_bytes / 2 ** 20:.1f}   {held}')


if __name__ == '__main__':
    main()
