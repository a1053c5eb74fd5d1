#!/usr/bin/env python3
"""Times the skinny-M GEMM (npm_sgemm_skinny, csrc/npm_skinny.hip) next to npm_sgemm on the same operands in the same process, on the
matrix products of a decode step at d 1024, hidden 4096, Hq 8 with Hkv 8 and 2, and then the step itself.

(a) Per GEMM.  The six products of TransformerDecoder.decode: the packed q/k/v projection (N 3072 at Hkv 8, 1536 at Hkv 2), a
projection with a bias (the cross-attention query), a projection with bias and residual (the two output projections), dense1
(bias + ReLU; npm_sgemm also stores the pre-activation, as the layer's call does) and dense2 (bias + residual), at M in {1, 2, 4, 8,
16, 32, 64} rows for both kernels and 128 for npm_sgemm alone.  "warm": the same weights every call (they stay in the Infinity
Cache); "cold": the weights rotate through copies that total 1 GiB, four times the Infinity Cache, so no call finds them in a
cache.  Time per call from HIP events around a window of back-to-back calls (launch gaps and the combine launch included: what a
user waits for); the windows of the two kernels ALTERNATE; min / median / max of 7 windows after an untimed one.  Weight bytes per
second (4 N K: what the product must read) as a fraction of 8 TB/s, the project's denominator, and of the ~6.3 TB/s this chip
streams.  The last lines say up to which M the skinny kernel is faster on every shape, warm and cold, by more than the spread of
both kernels' windows: that M is device.SKINNY_MAX_M.

(b) The step.  TransformerDecoder.decode at B in {1, 8, 64}, Hkv 8 and 2, L ~ 2048 with device.SKINNY_GEMM on and off, alternating
(7 windows of 20 steps each), and the per-kernel times of device.KernelTimer for both.

    python tools/skinny_gemm_bench.py > profiles/r11_skinny_gemm_bench.log
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DENOM_TBS, STREAM_TBS = 8.0, 6.3
ARENA_BYTES = 1 << 30          # four times the Infinity Cache
BIAS, RESIDUAL, RELU_SAVE, RELU = 1, 2, 4, 16
ROWS = (1, 2, 4, 8, 16, 32, 64)
# name, layout, N, K, epilogue of the skinny call, epilogue of the npm_sgemm call
SHAPES = (('qkv Hkv8', 'NT', 3072, 1024, BIAS, BIAS), ('qkv Hkv2', 'NT', 1536, 1024, BIAS, BIAS),
          ('q proj', 'NT', 1024, 1024, BIAS, BIAS), ('out proj', 'NT', 1024, 1024, BIAS | RESIDUAL, BIAS | RESIDUAL),
          ('dense1', 'NN', 4096, 1024, BIAS | RELU, BIAS | RELU_SAVE), ('dense2', 'NN', 1024, 4096, BIAS | RESIDUAL, BIAS | RESIDUAL))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=3.0, help='calls per window are sized so that a window lasts about this long')
    ap.add_argument('--no-gemm', action='store_true', help='skip part (a)')
    ap.add_argument('--no-step', action='store_true', help='skip part (b)')
    a = ap.parse_args()

    import np_modeling_amd as npm
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    try:
        head = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True,
                              cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip() or 'unknown'
    except OSError:
        head = 'unknown'
    print(f'skinny_gemm_bench: commit {head} (+ working tree), sources {_C.source_id()}; {a.windows} windows of ~{a.window_ms} ms per '
          f'kernel, alternating, after one untimed window each; times in microseconds per call', flush=True)

    def window(fn, calls):
        start = D.Event().record()
        for i in range(calls):
            fn(i)
        stop = D.Event().record()
        stop.synchronize()
        return start.elapsed_ms(stop) * 1e3 / calls

    def measure(fns):
        """min / median / max per function, the functions' windows alternating."""
        calls = []
        for fn in fns:
            window(fn, 8)                                         # untimed: code objects, first touch
            us = window(fn, 8)
            calls.append(int(max(8, min(2000, a.window_ms * 1e3 / max(us, 1.0)))))
            window(fn, calls[-1])
        times = [[] for _ in fns]
        for _ in range(a.windows):
            for t, fn, n in zip(times, fns, calls):
                t.append(window(fn, n))
        return [(min(t), sorted(t)[len(t) // 2], max(t)) for t in times]

    if not a.no_gemm:
        arena = D.full([ARENA_BYTES // 4], 0.01)
        x = D.from_host((0.1 * np.random.default_rng(0).standard_normal([128, 4096])).astype(np.float32))
        out, aux, res = D.empty([128, 4096]), D.empty([128, 4096]), D.full([128, 4096], 0.5)
        bias = D.full([4096], 0.25)
        print(f'{"product":>9} {"lay":>3} {"N":>5} {"K":>5} {"M":>3} {"state":>5} {"splits":>6} | {"skinny min/med/max":>24} {"of 8":>6} {"of 6.3":>6} | '
              f'{"npm_sgemm min/med/max":>24} | {"speedup":>7} {"clear":>5}', flush=True)
        wins = {}                                                 # M -> skinny faster beyond both spreads on every shape and state
        for name, layout, n, k, epi_skinny, epi_sgemm in SHAPES:
            floats = n * k
            slots = ARENA_BYTES // 4 // floats
            splits = lib.npm_sgemm_skinny_splits(n, k, int(layout == 'NT'))
            for m in ROWS + (128,):
                def desc(epilogue):
                    g = _C.npm_gemm()
                    g.trans_b, g.m, g.n, g.k, g.batch0, g.batch1 = int(layout == 'NT'), m, n, k, 1, 1
                    g.a, g.lda, g.ldb, g.c, g.ldc, g.alpha = x.ptr, k, k if layout == 'NT' else n, out.ptr, n, 1.0
                    g.epilogue, g.bias, g.residual, g.ldr = epilogue, bias.ptr, res.ptr if epilogue & RESIDUAL else None, n
                    if epilogue & RELU_SAVE:
                        g.aux, g.ldaux = aux.ptr, n
                    return g
                gs, gg = desc(epi_skinny), desc(epi_sgemm)

                def run(entry, g, what, rotate):
                    def fn(i):
                        g.b = arena.ptr + (4 * floats * (i % slots) if rotate else 0)
                        _C.check(entry(C.byref(g)), what)
                    return fn

                for state, rotate in (('warm', False), ('cold', True)):
                    sgemm = run(lib.npm_sgemm, gg, 'npm_sgemm', rotate)
                    if m > _C.SKINNY_MAX_M:
                        (base,) = measure([sgemm])
                        print(f'{name:>9} {layout:>3} {n:5d} {k:5d} {m:3d} {state:>5} {"":>6} | {"":>24} {"":>6} {"":>6} | '
                              f'{base[0]:8.1f}{base[1]:8.1f}{base[2]:8.1f} |', flush=True)
                        continue
                    sk, base = measure([run(lib.npm_sgemm_skinny, gs, 'npm_sgemm_skinny', rotate), sgemm])
                    tbs = 4.0 * floats / sk[1] / 1e6              # bytes / us -> TB/s
                    clear = sk[2] < base[0]                       # faster by more than the spread of both
                    wins[m] = wins.get(m, True) and clear
                    print(f'{name:>9} {layout:>3} {n:5d} {k:5d} {m:3d} {state:>5} {splits:6d} | {sk[0]:8.1f}{sk[1]:8.1f}{sk[2]:8.1f} '
                          f'{tbs / DENOM_TBS:6.3f} {tbs / STREAM_TBS:6.3f} | {base[0]:8.1f}{base[1]:8.1f}{base[2]:8.1f} | '
                          f'{base[1] / sk[1]:6.2f}x {"yes" if clear else "NO":>5}', flush=True)
        threshold = 0
        for m in ROWS:
            if not wins[m]:
                break
            threshold = m
        print(f'skinny faster than npm_sgemm beyond both spreads on all six products, warm and cold, at M in '
              f'{[m for m in ROWS if wins[m]]}; largest M with every smaller M included: {threshold} (device.SKINNY_MAX_M is '
              f'{D.SKINNY_MAX_M})', flush=True)
        del arena, x, out, aux, res, bias
        D.trim_pool()

    if a.no_step:
        return
    f, hidden, length, steps = 1024, 4096, 2048, 20
    for hkv in (8, 2):
        for b in (1, 8, 64):
            np.random.seed(0)
            layer = npm.layers.TransformerDecoder(num_heads=8, hidden_units=hidden, norm_first=True, num_kv_heads=hkv, causal=True)
            rng = np.random.default_rng(1)
            kv = rng.standard_normal([b, 128, f]).astype(np.float32)
            layer(np.zeros([b, 2, f], dtype=np.float32), kv)
            state = layer.start_decoding(kv, length + 1024)
            layer.decode((0.1 * rng.standard_normal([b, length, f])).astype(np.float32), state)      # prefill
            tok = (0.1 * rng.standard_normal([b, 1, f])).astype(np.float32)

            def step_window(on):
                D.SKINNY_GEMM = on
                start = D.Event().record()
                for _ in range(steps):
                    layer.decode(tok, state)
                stop = D.Event().record()
                stop.synchronize()
                return start.elapsed_ms(stop) * 1e3 / steps

            times = {True: [], False: []}
            for on in (True, False):
                step_window(on)                                   # untimed
            for _ in range(a.windows):
                for on in (True, False):
                    times[on].append(step_window(on))
            for on in (True, False):
                D.SKINNY_GEMM = on
                with D.KernelTimer() as timer:
                    for _ in range(steps):
                        layer.decode(tok, state)
                rec = timer.summary()
                total = sum(r['ms'] for r in rec.values())
                gemm = sum(r['ms'] for n, r in rec.items() if n.startswith('sgemm_'))
                att = sum(r['ms'] for n, r in rec.items() if n in ('mha_decode', 'kv_append'))
                t = sorted(times[on])
                parts = ', '.join(f'{n} {r["ms"] * 1e3 / steps:.1f}' for n, r in sorted(rec.items(), key=lambda x: -x[1]['ms']))
                print(f'decode step d {f} Hq 8 Hkv {hkv} B {b} L {state.position} SKINNY_GEMM {"on " if on else "off"}: '
                      f'{t[0]:.1f} / {t[len(t) // 2]:.1f} / {t[-1]:.1f} us per step (min / median / max of {a.windows} windows of {steps} '
                      f'steps); KernelTimer: GEMMs {gemm * 1e3 / steps:.1f} us, attention {att * 1e3 / steps:.1f} us = {att / total:.1%} of '
                      f'{total * 1e3 / steps:.1f} us; us per step: {parts}', flush=True)
            D.SKINNY_GEMM = True
            del layer, state
            D.trim_pool()


if __name__ == '__main__':
    main()
