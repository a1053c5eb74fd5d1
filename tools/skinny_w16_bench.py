#!/usr/bin/env python3
"""Times the skinny-M GEMM over fp16 weight copies (npm_sgemm_skinny_w16, csrc/npm_skinny.hip) next to npm_sgemm_skinny on the
fp32 weights, same activations, same process, on the matrix products of a decode step at d 1024, hidden 4096, Hq 8 with Hkv 8 and
2, and then the step itself with and without ``start_decoding(..., weights='f16')``.

(a) Per GEMM (``--part gemm``).  The six products of TransformerDecoder.decode at M in {1, 8, 16, 64} rows, COLD weights: both
kernels rotate through copies that total 1 GiB of fp32 weights (four times the Infinity Cache; the halves rotate through the same
number of copies), so no call finds its weights in a cache.  Time per call from HIP events around a window of back-to-back calls
(launch gaps and the combine launch included); the windows of the two kernels ALTERNATE; min / median / max of 7 windows after an
untimed one.  Reported: the ratio w16 / fp32 of the medians (below 1: the halves are faster), whether the two spreads are
disjoint, and the weight bytes per second each kernel moves (2 N K and 4 N K) in GB/s and as a fraction of 8 TB/s.

(b) The step (``--part step``).  TransformerDecoder.decode at B in {1, 8, 64}, Hkv 8 and 2, L ~ 2048, with and without the half
weights, alternating (7 windows of 20 steps each), and the per-kernel times of device.KernelTimer for both.

Without ``--part`` the tool is the driver: it runs each part in a child process of its own under its own time limit, stops at the
first part that fails or runs out of time, and writes everything to ``--out`` (default profiles/r16_skinny_w16_bench.log).

    python tools/skinny_w16_bench.py
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DENOM_TBS = 8.0
ARENA_BYTES = 1 << 30          # fp32 copies: four times the Infinity Cache
BIAS, RESIDUAL, RELU = 1, 2, 16
ROWS = (1, 8, 16, 64)
# name, layout, N, K, epilogue (what the decode path asks of the skinny kernels)
SHAPES = (('qkv Hkv8', 'NT', 3072, 1024, BIAS), ('qkv Hkv2', 'NT', 1536, 1024, BIAS), ('q proj', 'NT', 1024, 1024, BIAS),
          ('out proj', 'NT', 1024, 1024, BIAS | RESIDUAL), ('dense1', 'NN', 4096, 1024, BIAS | RELU), ('dense2', 'NN', 1024, 4096, BIAS | RESIDUAL))
PART_LIMIT_S = {'gemm': 240, 'step': 300}


def window(D, fn, calls):
    start = D.Event().record()
    for i in range(calls):
        fn(i)
    stop = D.Event().record()
    stop.synchronize()
    return start.elapsed_ms(stop) * 1e3 / calls


def measure(D, fns, windows, window_ms):
    """min / median / max per function, the functions' windows alternating."""
    calls = []
    for fn in fns:
        window(D, fn, 8)                                              # untimed: code objects, first touch
        us = window(D, fn, 8)
        calls.append(int(max(8, min(2000, window_ms * 1e3 / max(us, 1.0)))))
        window(D, fn, calls[-1])
    times = [[] for _ in fns]
    for _ in range(windows):
        for t, fn, n in zip(times, fns, calls):
            t.append(window(D, fn, n))
    return [(min(t), sorted(t)[len(t) // 2], max(t)) for t in times]


def part_gemm(a) -> None:
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    arena = D.full([ARENA_BYTES // 4], 0.01)
    halves = D.HalfBuffer([ARENA_BYTES // 4])
    _C.check(lib.npm_cvt_f32_f16(arena.ptr, 1 << 20, halves.ptr, 1 << 20, ARENA_BYTES // 4 >> 20, 1 << 20), 'npm_cvt_f32_f16')
    x = D.from_host((0.1 * np.random.default_rng(0).standard_normal([64, 4096])).astype(np.float32))
    out, res, bias = D.empty([64, 4096]), D.full([64, 4096], 0.5), D.full([4096], 0.25)
    print(f'{"product":>9} {"lay":>3} {"N":>5} {"K":>5} {"M":>3} {"splits":>6} | {"fp32 skinny min/med/max":>24} {"GB/s":>6} {"of 8":>6} | '
          f'{"w16 min/med/max":>24} {"GB/s":>6} {"of 8":>6} | {"w16/fp32":>8} {"clear":>6}', flush=True)
    for name, layout, n, k, epilogue in SHAPES:
        elems = n * k
        slots = ARENA_BYTES // 4 // elems
        splits = lib.npm_sgemm_skinny_splits(n, k, int(layout == 'NT'))
        for m in ROWS:
            def run(entry, what, base, itemsize):
                g = _C.npm_gemm()
                g.trans_b, g.m, g.n, g.k, g.batch0, g.batch1 = int(layout == 'NT'), m, n, k, 1, 1
                g.a, g.lda, g.ldb, g.c, g.ldc, g.alpha = x.ptr, k, k if layout == 'NT' else n, out.ptr, n, 1.0
                g.epilogue, g.bias, g.residual, g.ldr = epilogue, bias.ptr, res.ptr if epilogue & RESIDUAL else None, n

                def fn(i):
                    g.b = base + itemsize * elems * (i % slots)
                    _C.check(entry(C.byref(g)), what)
                return fn

            f32, w16 = measure(D, [run(lib.npm_sgemm_skinny, 'npm_sgemm_skinny', arena.ptr, 4),
                                   run(lib.npm_sgemm_skinny_w16, 'npm_sgemm_skinny_w16', halves.ptr, 2)], a.windows, a.window_ms)
            gbs32, gbs16 = 4.0 * elems / f32[1] / 1e3, 2.0 * elems / w16[1] / 1e3          # bytes / us -> GB/s
            clear = 'faster' if w16[2] < f32[0] else ('SLOWER' if w16[0] > f32[2] else 'no')
            print(f'{name:>9} {layout:>3} {n:5d} {k:5d} {m:3d} {splits:6d} | {f32[0]:8.1f}{f32[1]:8.1f}{f32[2]:8.1f} {gbs32:6.0f} '
                  f'{gbs32 / 1e3 / DENOM_TBS:6.3f} | {w16[0]:8.1f}{w16[1]:8.1f}{w16[2]:8.1f} {gbs16:6.0f} {gbs16 / 1e3 / DENOM_TBS:6.3f} | '
                  f'{w16[1] / f32[1]:8.3f} {clear:>6}', flush=True)
    print(f'last kernel: {_C.last_skinny_kernel()}', flush=True)


def part_step(a) -> None:
    import np_modeling_amd as npm
    from np_modeling_amd import device as D
    f, hidden, length, steps = 1024, 4096, 2048, 20
    for hkv in (8, 2):
        for b in (1, 8, 64):
            np.random.seed(0)
            layer = npm.layers.TransformerDecoder(num_heads=8, hidden_units=hidden, norm_first=True, num_kv_heads=hkv, causal=True)
            rng = np.random.default_rng(1)
            kv = rng.standard_normal([b, 128, f]).astype(np.float32)
            layer(np.zeros([b, 2, f], dtype=np.float32), kv)
            states = {}
            for weights in (None, 'f16'):
                states[weights] = layer.start_decoding(kv, length + 1024, weights=weights)
                layer.decode((0.1 * rng.standard_normal([b, length, f])).astype(np.float32), states[weights])      # prefill
            tok = (0.1 * rng.standard_normal([b, 1, f])).astype(np.float32)

            def step_window(weights):
                return window(D, lambda i: layer.decode(tok, states[weights]), steps)

            times = {None: [], 'f16': []}
            for weights in times:
                step_window(weights)                                  # untimed
            for _ in range(a.windows):
                for weights in times:
                    times[weights].append(step_window(weights))
            for weights in times:
                with D.KernelTimer() as timer:
                    for _ in range(steps):
                        layer.decode(tok, states[weights])
                rec = timer.summary()
                total = sum(r['ms'] for r in rec.values())
                gemm = sum(r['ms'] for n, r in rec.items() if n.startswith('sgemm_'))
                t = sorted(times[weights])
                parts = ', '.join(f'{n} {r["ms"] * 1e3 / steps:.1f}' for n, r in sorted(rec.items(), key=lambda x: -x[1]['ms']))
                print(f'decode step d {f} Hq 8 Hkv {hkv} B {b} L {states[weights].position} weights {str(weights):>4}: '
                      f'{t[0]:.1f} / {t[len(t) // 2]:.1f} / {t[-1]:.1f} us per step (min / median / max of {a.windows} windows of {steps} '
                      f'steps); KernelTimer: GEMMs {gemm * 1e3 / steps:.1f} us of {total * 1e3 / steps:.1f} us; us per step: {parts}', flush=True)
            med = {w: sorted(t)[len(t) // 2] for w, t in times.items()}
            print(f'decode step Hkv {hkv} B {b}: f16 weights / fp32 weights = {med["f16"] / med[None]:.3f}', flush=True)
            del layer, states
            D.trim_pool()


def drive(a) -> int:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    from np_modeling_amd import _C
    with open(a.out, 'w') as log:
        def say(text):
            print(text, flush=True)
            log.write(text + '\n')
            log.flush()

        say(f'skinny_w16_bench: sources {_C.source_id()}; {a.windows} windows of ~{a.window_ms} ms per kernel, '
            f'alternating, after one untimed window each; cold weights; times in microseconds per call')
        for part in ('gemm', 'step'):
            if part in a.skip:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), '--part', part, '--windows', str(a.windows), '--window-ms', str(a.window_ms)]
            try:                                                      # a part that faults, aborts or hangs ends the run: nothing is started after it
                proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=PART_LIMIT_S[part], cwd=ROOT)
            except subprocess.TimeoutExpired as err:
                say((err.stdout or b'').decode() if isinstance(err.stdout, bytes) else (err.stdout or ''))
                say(f'part {part}: no result within {PART_LIMIT_S[part]} s; stopping')
                return 124
            say(proc.stdout.rstrip('\n'))
            if proc.returncode != 0:
                say(f'part {part}: exit status {proc.returncode}; stopping')
                return proc.returncode
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=3.0, help='calls per window are sized so that a window lasts about this long')
    ap.add_argument('--part', choices=('gemm', 'step'), help='run one part in this process (the driver does this)')
    ap.add_argument('--skip', nargs='*', default=[], choices=('gemm', 'step'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r16_skinny_w16_bench.log'))
    a = ap.parse_args()
    if a.part == 'gemm':
        part_gemm(a)
    elif a.part == 'step':
        part_step(a)
    else:
        return drive(a)
    return 0


if __name__ == '__main__':
    sys.exit(main())
