#!/usr/bin/env python3
"""Times the rotary position embedding kernel (npm_rope, csrc/npm_rope.hip) and what it adds to a decode step.

(a) The kernel alone at H 8 + Hkv 8 = 16 heads of D 128 (row pitch 2048 floats: every element of the buffer is rotated), at
B 64 T 1 (a decode step: 512 KB), B 8 T 2048 (a prefill: 128 MB) and B 16 T 2048 (256 MB, the size of the Infinity Cache), next to
the project's in-place element-wise kernel npm_scale (alpha = 1) on the very same buffer in the same process, in alternating
windows.  Both read and write every element once; npm_rope also reads T rows of the two tables (1 / (2 heads) of the bytes, about
3 %), which stay in L2.  One more column: the same rows inside a packed [B, T, H + 2 Hkv, D] projection (pitch 3072), where the V
heads are skipped.  Time per call from HIP events around a window of back-to-back calls (launch gaps included), min / median / max
over the windows; bytes per second are the algorithm's bytes (8 per rotated element, plus the table rows for npm_rope).

(b) One TransformerDecoder.decode step at T 1, d 1024, 8 heads, hidden 4096, about 2048 cached rows, B in {1, 8, 64}, with and
without ``rope_base``, in alternating windows of steps on two layers with the same weights; then the per-kernel times of
device.KernelTimer for the rotating layer.

    python tools/rope_bench.py > profiles/r16_rope_bench.log
"""
import argparse
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEADS, D_HEAD, BASE = 16, 128, 1e4


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='64x1,8x2048,16x2048', help='B x T of the kernel measurement')
    ap.add_argument('--b', default='1,8,64', help='batch sizes of the decode step')
    ap.add_argument('--l', type=int, default=2048, help='cached rows before the timed decode steps')
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=8.0, help='calls per window are sized so that a window lasts about this long')
    ap.add_argument('--steps', type=int, default=20, help='decode steps per window')
    ap.add_argument('--no-step', action='store_true', help='skip the decode step')
    a = ap.parse_args(argv)

    import np_modeling_amd as npm
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    try:
        head = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True,
                              cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip() or 'unknown'
    except OSError:
        head = 'unknown'
    print(f'rope_bench: commit {head} (+ working tree), sources {_C.source_id()}, {HEADS} heads of D {D_HEAD}; {a.windows} windows of '
          f'~{a.window_ms} ms per kernel, alternating, after untimed ones; times in microseconds per call', flush=True)

    def window(fn, calls):
        start = D.Event().record()
        for _ in range(calls):
            fn()
        stop = D.Event().record()
        stop.synchronize()
        return start.elapsed_ms(stop) * 1e3 / calls

    def measure(fns):
        """min / median / max per function over alternating windows."""
        calls = []
        for fn in fns:
            window(fn, 8)                                             # untimed: code objects, first touch
            us = window(fn, 8)
            calls.append(int(max(8, min(4000, a.window_ms * 1e3 / max(us, 1.0)))))
            window(fn, calls[-1])
        times = [[] for _ in fns]
        for _ in range(a.windows):
            for i, fn in enumerate(fns):
                times[i].append(window(fn, calls[i]))
        return [(min(t), sorted(t)[len(t) // 2], max(t)) for t in times]

    # ---- (a) the kernel alone -------------------------------------------------------------------------------------------------------
    row = HEADS * D_HEAD
    packed_row = row + 8 * D_HEAD                                         # H 8 + 2 Hkv 8 heads: the V heads behind q and k
    print(f'{"B":>3} {"T":>5} {"MB":>6} | {"npm_rope min/med/max":>26} {"TB/s":>6} | {"npm_scale min/med/max":>26} {"TB/s":>6} | '
          f'{"rope/scale":>10} {"expected":>8} | {"packed pitch med":>16} {"TB/s":>6}', flush=True)
    for shape in a.shapes.split(','):
        b, t = (int(v) for v in shape.split('x'))
        rows = b * t
        at = 1000 if t == 1 else 0                                        # a decode step sits somewhere inside the sequence
        table = D.RopeTable(D_HEAD, BASE).ensure(at + t)
        rng = np.random.default_rng(0)
        x = D.from_host(rng.standard_normal([min(rows, 4096), row]).astype(np.float32)) if rows <= 4096 else D.full([rows, row], 0.5)
        xp = D.full([rows, packed_row], 0.5)
        n = rows * row

        def run_rope(x=x, pitch=row):
            _C.check(lib.npm_rope(x.ptr, pitch, b, t, HEADS, D_HEAD, table.cos.ptr, table.sin.ptr, table.rows, at, None, 0), 'npm_rope')

        def run_scale():
            _C.check(lib.npm_scale(x.ptr, x.ptr, 1.0, n), 'npm_scale')

        rope, scale, packed = measure([run_rope, run_scale, lambda: run_rope(xp, packed_row)])
        table_bytes = 2 * t * (D_HEAD // 2) * 4
        rope_bytes, scale_bytes = 8.0 * n + table_bytes, 8.0 * n
        print(f'{b:3d} {t:5d} {4 * n / 2 ** 20:6.1f} | {rope[0]:8.1f} {rope[1]:8.1f} {rope[2]:8.1f} {rope_bytes / rope[1] / 1e6:6.2f} | '
              f'{scale[0]:8.1f} {scale[1]:8.1f} {scale[2]:8.1f} {scale_bytes / scale[1] / 1e6:6.2f} | {rope[1] / scale[1]:10.3f} '
              f'{1 + 1 / (2 * HEADS):8.3f} | {packed[1]:16.1f} {rope_bytes / packed[1] / 1e6:6.2f}', flush=True)
        del x, xp, table
        D.trim_pool()
    print('expected: the npm_scale time plus the tables\' share of the bytes (1 / (2 heads)), within the spread of the npm_scale rows',
          flush=True)

    if a.no_step:
        return
    # ---- (b) the decode step ----------------------------------------------------------------------------------------------------------
    f, hidden, length = 1024, 4096, a.l
    total_steps = 6 + (a.windows + 1) * a.steps * 2
    for b in (int(v) for v in a.b.split(',')):
        rng = np.random.default_rng(1)
        kv = rng.standard_normal([b, 128, f]).astype(np.float32)
        prompt = (0.1 * rng.standard_normal([b, length, f])).astype(np.float32)
        tok = D.from_host((0.1 * rng.standard_normal([b, 1, f])).astype(np.float32))
        layers = []
        for base in (None, BASE):
            np.random.seed(0)                                             # the same weights in both
            layer = npm.layers.TransformerDecoder(num_heads=8, hidden_units=hidden, norm_first=True, causal=True, rope_base=base)
            layer(np.zeros([b, 2, f], dtype=np.float32), kv)
            state = layer.start_decoding(kv, length + total_steps)
            layer.decode(prompt, state)                                   # prefill
            for _ in range(3):
                layer.decode(tok, state)
            layers.append((layer, state))
        times = [[], []]
        for w in range(a.windows + 1):                                    # the first pair of windows is not counted
            for i, (layer, state) in enumerate(layers):
                us = window(lambda: layer.decode(tok, state), a.steps)
                if w:
                    times[i].append(us)
        plain, rope = ((min(t), sorted(t)[len(t) // 2], max(t)) for t in times)
        layer, state = layers[1]
        with D.KernelTimer() as timer:
            for _ in range(a.steps):
                layer.decode(tok, state)
        rec = timer.summary()
        parts = ', '.join(f'{n} {r["ms"] * 1e3 / a.steps:.1f} ({r["launches"] // a.steps})' for n, r in sorted(rec.items(), key=lambda x: -x[1]['ms']))
        print(f'decode step d {f} H 8 D 128 hidden {hidden} B {b} L {state.position}: without rope {plain[0]:.1f} / {plain[1]:.1f} / '
              f'{plain[2]:.1f} us per step (min / median / max of {a.windows} windows of {a.steps} steps), with rope_base {rope[0]:.1f} / '
              f'{rope[1]:.1f} / {rope[2]:.1f}: {rope[1] - plain[1]:+.1f} us ({rope[1] / plain[1] - 1:+.1%}); kernels of the rotating layer, us '
              f'per step under the event timer (launches): {parts}', flush=True)
        del layers, layer, state
        D.trim_pool()


if __name__ == '__main__':
    main()
