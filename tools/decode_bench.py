#!/usr/bin/env python3
"""Times incremental decoding's attention (npm_mha_decode_fwd, csrc/npm_decode.hip) alone at T = 1 new token, Hq 8, D 128,
B in {1, 8, 64} x L in {512, 2048, 8192} x Hkv in {8, 2, 1}, next to the only route the library had for the same result before
the kernel existed: npm_mha_core_fwd_grouped with seq_q = 1 (no mask is needed at T = 1), in the same process.

What is reported.  Time per call from HIP events around a window of back-to-back calls (launch gaps and, where the keys are
split, the combine launch included: what a user waits for), min / median / max over the windows.  K / V bytes per second
(2 B L Hkv D 4 bytes: what the algorithm must read; q, ctx and the partials are not counted) as a fraction of 8 TB/s, the
project's denominator, with the fraction of the ~6.3 TB/s this chip streams beside it.

Cache state.  "cold": every call of a window reads a different K / V slice of two arenas that are together far larger than the
256 MB Infinity Cache (a single K / V pair larger than that is its own arena), so no call finds its keys in a cache.  "hot": the
same slice every call -- what a cache of a size that fits the caches gives.  The baseline is timed cold.

Both load policies of the decode kernel are timed cold (NPM_TUNE_DECODE_NT = 2 plain, 1 nontemporal) beside the default (0:
nontemporal from 32 MB of K up); the "decode cold" columns and the speedup are the default's.

Last, one TransformerDecoder.decode step (d 1024, 8 heads, hidden 4096, L 2048) with the per-kernel times of device.KernelTimer:
attention's share of the step is what sizes the skinny-M GEMM follow-up.

    python tools/decode_bench.py > profiles/r08_decode_bench.log
    rocprofv3 --kernel-trace --stats -d DIR -o decode -- python tools/decode_bench.py --b 64 --l 8192 --kv 8 --no-step
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DENOM_TBS, STREAM_TBS = 8.0, 6.3
ARENA_BYTES = 1 << 30          # per arena (K and V each): four times the Infinity Cache


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--b', default='1,8,64')
    ap.add_argument('--l', default='512,2048,8192')
    ap.add_argument('--kv', default='8,2,1')
    ap.add_argument('--h', type=int, default=8)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=8.0, help='calls per window are sized so that a window lasts about this long')
    ap.add_argument('--no-step', action='store_true', help='skip the TransformerDecoder.decode step')
    a = ap.parse_args()

    import np_modeling_amd as npm
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    h, d = a.h, a.d
    scale = 1.0 / np.sqrt(d)
    try:
        head = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True,
                              cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip() or 'unknown'
    except OSError:
        head = 'unknown'
    print(f'decode_bench: commit {head} (+ working tree), sources {_C.source_id()}, Hq {h} D {d} T 1; {a.windows} windows of '
          f'~{a.window_ms} ms after one untimed window; times in microseconds per call', flush=True)

    def window(fn, calls):
        start = D.Event().record()
        for i in range(calls):
            fn(i)
        stop = D.Event().record()
        stop.synchronize()
        return start.elapsed_ms(stop) * 1e3 / calls

    def measure(fn):
        calls = 8
        us = window(fn, calls)                                    # untimed: code objects, first touch
        us = window(fn, calls)
        calls = int(max(8, min(4000, a.window_ms * 1e3 / max(us, 1.0))))
        window(fn, calls)
        t = sorted(window(fn, calls) for _ in range(a.windows))
        return t[0], t[len(t) // 2], t[-1]

    print(f'{"B":>3} {"L":>5} {"Hkv":>3} {"splits":>6} | {"decode cold min/med/max":>26} {"of 8":>6} {"of 6.3":>6} | {"plain med":>9} {"nt med":>8} | '
          f'{"hot med":>8} | {"baseline cold min/med/max":>28} | {"speedup":>7}', flush=True)
    slower = []
    for b in (int(x) for x in a.b.split(',')):
        for length in (int(x) for x in a.l.split(',')):
            for hkv in (int(x) for x in a.kv.split(',')):
                floats = b * length * hkv * d                     # one of K, V
                arena = max(ARENA_BYTES // 4, floats)
                slots = max(1, arena // floats)
                ka, va = D.full([arena], 0.01), D.full([arena], 0.02)
                q = D.from_host(np.random.default_rng(0).standard_normal([b, 1, h, d]).astype(np.float32))
                ctx, lse = D.empty([b, 1, h, d]), D.empty([b, h, 1])
                dec = _C.npm_mha_decode()
                dec.batch, dec.heads, dec.kv_heads, dec.new_tokens, dec.kv_len, dec.head_dim = b, h, hkv, 1, length, d
                dec.causal, dec.scale = 1, scale
                dec.q, dec.q_pitch, dec.ctx, dec.ctx_pitch, dec.lse = q.ptr, h * d, ctx.ptr, h * d, lse.ptr
                dec.k_pitch = dec.v_pitch = hkv * d
                dec.k_stride_b = dec.v_stride_b = length * hkv * d
                core = _C.npm_mha_core()
                core.batch, core.heads, core.seq_q, core.seq_kv, core.head_dim, core.scale = b, h, 1, length, d, scale
                core.q, core.q_pitch, core.k_pitch, core.v_pitch = q.ptr, h * d, hkv * d, hkv * d
                core.ctx, core.ctx_pitch, core.lse = ctx.ptr, h * d, lse.ptr

                def run_decode(i, rotate=True):
                    off = 4 * floats * (i % slots if rotate else 0)
                    dec.k, dec.v = ka.ptr + off, va.ptr + off
                    _C.check(lib.npm_mha_decode_fwd(C.byref(dec)), 'npm_mha_decode_fwd')

                def run_core(i):
                    off = 4 * floats * (i % slots)
                    core.k, core.v = ka.ptr + off, va.ptr + off
                    _C.check(lib.npm_mha_core_fwd_grouped(C.byref(core), hkv), 'npm_mha_core_fwd_grouped')

                cold = measure(run_decode)
                hot = measure(lambda i: run_decode(i, rotate=False))
                _C.check(lib.npm_set_tuning(_C.TUNE_DECODE_NT, 2), 'npm_set_tuning')
                plain = measure(run_decode)
                _C.check(lib.npm_set_tuning(_C.TUNE_DECODE_NT, 1), 'npm_set_tuning')
                nt = measure(run_decode)
                _C.check(lib.npm_set_tuning(_C.TUNE_DECODE_NT, 0), 'npm_set_tuning')
                base = measure(run_core)
                splits = lib.npm_mha_decode_splits(b, hkv, length)
                tbs = 8.0 * floats / cold[1] / 1e6                # bytes / us -> TB/s
                print(f'{b:3d} {length:5d} {hkv:3d} {splits:6d} | {cold[0]:8.1f} {cold[1]:8.1f} {cold[2]:8.1f} {tbs / DENOM_TBS:6.3f} '
                      f'{tbs / STREAM_TBS:6.3f} | {plain[1]:9.1f} {nt[1]:8.1f} | {hot[1]:8.1f} | {base[0]:9.1f} {base[1]:8.1f} {base[2]:8.1f} | '
                      f'{base[1] / cold[1]:6.2f}x', flush=True)
                if cold[0] > base[2]:                             # slower beyond the spread both report
                    slower.append((b, length, hkv))
                del ka, va
                D.trim_pool()
    print('decode kernel slower than the baseline beyond the spread at:', slower or 'no shape', flush=True)

    if a.no_step:
        return
    # one decode step of a decoder layer: attention against everything else
    f, hidden, length = 1024, 4096, 2048
    for hkv in (8, 2):
        for b in (1, 8, 64):
            np.random.seed(0)
            layer = npm.layers.TransformerDecoder(num_heads=8, hidden_units=hidden, norm_first=True, num_kv_heads=hkv, causal=True)
            rng = np.random.default_rng(1)
            kv = rng.standard_normal([b, 128, f]).astype(np.float32)
            layer(np.zeros([b, 2, f], dtype=np.float32), kv)
            state = layer.start_decoding(kv, length + 64)
            layer.decode((0.1 * rng.standard_normal([b, length, f])).astype(np.float32), state)      # prefill
            tok = (0.1 * rng.standard_normal([b, 1, f])).astype(np.float32)
            for _ in range(3):
                layer.decode(tok, state)
            steps = 20
            start = D.Event().record()
            for _ in range(steps):
                layer.decode(tok, state)
            stop = D.Event().record()
            stop.synchronize()
            step_us = start.elapsed_ms(stop) * 1e3 / steps
            with D.KernelTimer() as timer:
                for _ in range(steps):
                    layer.decode(tok, state)
            rec = timer.summary()
            total = sum(r['ms'] for r in rec.values())
            att = sum(r['ms'] for n, r in rec.items() if n in ('mha_decode', 'kv_append'))
            parts = ', '.join(f'{n} {r["ms"] * 1e3 / steps:.1f}' for n, r in sorted(rec.items(), key=lambda x: -x[1]['ms']))
            print(f'decode step d {f} Hq 8 Hkv {hkv} B {b} L {state.position}: {step_us:.1f} us per step (host clock of the stream, '
                  f'{len(rec)} kernel kinds); attention (mha_decode + kv_append) {att / total:.1%} of the kernel time; us per step: '
                  f'{parts}', flush=True)
            del layer, state
            D.trim_pool()


if __name__ == '__main__':
    main()
