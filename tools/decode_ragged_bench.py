#!/usr/bin/env python3
"""Times the decode attention of a RAGGED batch (npm_mha_decode_fwd_varlen, csrc/npm_decode.hip) at T = 1 new token, Hq 8, D 128,
B 64, Lmax 8192, Hkv in {8, 1}, with the method of tools/decode_bench.py: time per call from HIP events around a window of
back-to-back calls (the combine launch included), min / median / max over the windows; "cold" K / V (every call of a window reads
a different slice of two arenas far larger than the 256 MB Infinity Cache; a K / V pair larger than that is its own arena).  The
cache layout is [B, Lmax, Hkv, D] throughout: only the lengths differ between the rows.

Per shape, in one process:
  (a) npm_mha_decode_fwd at L = Lmax               what holding such a batch costs without per-sequence lengths: the baseline
  (b) varlen, every length = Lmax                  same work, same partition as (a): must lie within (a)'s own spread
  (c) varlen, lengths uniform in 1 .. Lmax (seeded), and skewed (one sequence at Lmax, the others at Lmax / 16)
  (d) npm_mha_decode_fwd at the uniform length with (c)'s total number of keys: what "cost follows the sum of the lengths" means
  (e) (a) again, beside the number profiles/r08_decode_bench.log holds for the shape
and the ratios (b) / (a), (c) / (a), (c) / (d) of the medians.

    python tools/decode_ragged_bench.py > profiles/r09_decode_ragged_bench.log
    rocprofv3 --kernel-trace --stats -d DIR -o ragged -- python tools/decode_ragged_bench.py --kv 8 --only skewed
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARENA_BYTES = 1 << 30
R08 = {8: (638.3, 662.6, 663.6), 1: (94.7, 95.2, 95.5)}      # profiles/r08_decode_bench.log, B 64 L 8192: decode cold min / med / max


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--b', type=int, default=64)
    ap.add_argument('--lmax', type=int, default=8192)
    ap.add_argument('--kv', default='8,1')
    ap.add_argument('--h', type=int, default=8)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=8.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--only', default='', help='time one row only (a, b, uniform, skewed): for a profiler run')
    a = ap.parse_args()

    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    b, lmax, h, d = a.b, a.lmax, a.h, a.d
    scale = 1.0 / np.sqrt(d)
    print(f'decode_ragged_bench: sources {_C.source_id()}, B {b} Lmax {lmax} Hq {h} D {d} T 1; {a.windows} windows of ~{a.window_ms} ms '
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
    draws = {'uniform': rng.integers(1, lmax + 1, b), 'skewed': np.array([lmax] + [lmax // 16] * (b - 1))}
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
        dec.k_stride_b = dec.v_stride_b = lmax * hkv * d

        def uniform(length):
            def run(i):
                off = 4 * floats * (i % slots)
                dec.k, dec.v, dec.kv_len = ka.ptr + off, va.ptr + off, length
                _C.check(lib.npm_mha_decode_fwd(C.byref(dec)), 'npm_mha_decode_fwd')
            return run

        def varlen(lengths):
            dev = D.bytes_from_host(np.ascontiguousarray(np.asarray(lengths, dtype=np.int32)))

            def run(i, dev=dev):
                off = 4 * floats * (i % slots)
                dec.k, dec.v, dec.kv_len = ka.ptr + off, va.ptr + off, lmax
                _C.check(lib.npm_mha_decode_fwd_varlen(C.byref(dec), dev.ptr, None), 'npm_mha_decode_fwd_varlen')
            return run

        def row(tag, t, extra=''):
            print(f'Hkv {hkv} {tag:<44} {t[0]:8.1f} {t[1]:8.1f} {t[2]:8.1f}{extra}', flush=True)

        splits = lib.npm_mha_decode_splits(b, hkv, lmax)
        print(f'Hkv {hkv}: splits {splits} (of Lmax), {slots} K / V slice(s) of {8.0 * floats / 2 ** 20:.0f} MB;'
              f'{"":>22} min      med      max', flush=True)
        if a.only in ('', 'a'):
            ta = measure(uniform(lmax))
            row(f'(a) decode_fwd L = {lmax}', ta, f'   spread {(ta[2] - ta[0]) / ta[1]:.1%}')
        if a.only in ('', 'b'):
            tb = measure(varlen([lmax] * b))
            row(f'(b) varlen, all lengths {lmax}', tb, f'   (b) / (a) {tb[1] / ta[1]:.3f}; min (b) {"<=" if tb[0] <= ta[2] else ">"} max (a)' if not a.only else '')
        for name, lengths in draws.items():
            if a.only not in ('', name):
                continue
            total = int(lengths.sum())
            mean = max(1, round(total / b))
            tc = measure(varlen(lengths))
            if a.only:
                row(f'(c) varlen {name}: sum {total}', tc)
                continue
            td = measure(uniform(mean))
            sd = lib.npm_mha_decode_splits(b, hkv, mean)
            row(f'(c) varlen {name}: sum {total} = {total / (b * lmax):.3f} B Lmax', tc, f'   (c) / (a) {tc[1] / ta[1]:.3f}')
            row(f'(d) decode_fwd L = {mean} (same keys, splits {sd})', td, f'   (c) / (d) {tc[1] / td[1]:.3f}')
        if not a.only:
            te = measure(uniform(lmax))
            ref = R08.get(hkv) if (b, lmax, h, d) == (64, 8192, 8, 128) else None
            row('(e) (a) again', te, f'   r08 log: {ref[0]:.1f} {ref[1]:.1f} {ref[2]:.1f}' if ref else '')
        del ka, va
        D.trim_pool()


if __name__ == '__main__':
    main()
