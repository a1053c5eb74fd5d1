#!/usr/bin/env python3
"""Times token sampling (npm_sample_rows, csrc/npm_sample.hip) on cold logits against the project's row softmax on the same buffer.

B in {1, 8, 64} x V in {32000, 128256}; greedy, top-k 50, top-p 0.9 and both (temperature 0.8 where it samples).  Cold: the
[B, V] logit matrices of successive calls walk through one 512 MB region (twice the Infinity Cache), so no call finds its rows
in L2 or the Infinity Cache.  The yardstick is npm_softmax_fwd over the very same matrices in the same process, in alternating
windows: it reads a row once and writes it once, where the sampler reads it once from HBM, then several times from LDS (V <=
32768) or L2, and writes 12 bytes.  Time per call from HIP events around a window of back-to-back calls (launch gaps included),
min / median / max over the windows.

    python tools/sample_bench.py > profiles/sample_bench.log
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = [('greedy', 0.0, 0, 1.0), ('top-k 50', 0.8, 50, 1.0), ('top-p 0.9', 0.8, 0, 0.9), ('k 50 + p 0.9', 0.8, 50, 0.9)]


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--b', default='1,8,64')
    ap.add_argument('--v', default='32000,128256')
    ap.add_argument('--region-mb', type=int, default=512)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--calls', type=int, default=64, help='calls per window')
    a = ap.parse_args(argv)

    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    print(f'sample_bench: sources {_C.source_id()}; {a.windows} windows of {a.calls} calls per kernel, alternating, after untimed ones; '
          f'logits walk a {a.region_mb} MB region; microseconds per call', flush=True)
    region_floats = a.region_mb * (1 << 20) // 4
    chunk = 1 << 22
    region = D.empty([region_floats])
    rng = np.random.default_rng(0)
    noise = D.from_host((4 * rng.standard_normal(chunk)).astype(np.float32))
    for at in range(0, region_floats, chunk):
        _C.check(lib.npm_d2d(region.ptr + 4 * at, noise.ptr, 4 * min(chunk, region_floats - at)), 'npm_d2d')
    scratch = D.empty([64 * 128256])

    def window(fn, calls):
        start = D.Event().record()
        for _ in range(calls):
            fn()
        stop = D.Event().record()
        stop.synchronize()
        return start.elapsed_ms(stop) * 1e3 / calls

    print(f'{"B":>3} {"V":>7} {"mode":>13} | {"npm_sample_rows min/med/max":>30} | {"npm_softmax_fwd min/med/max":>30} | {"sample/softmax":>14} | kernel')
    for b in (int(v) for v in a.b.split(',')):
        for vocab in (int(v) for v in a.v.split(',')):
            slots = region_floats // (b * vocab)
            for name, t, k, p in MODES:
                params = D.bytes_from_host(np.concatenate([
                    np.arange(b, dtype=np.uint64).view(np.uint8), np.zeros(b, dtype=np.uint64).view(np.uint8),
                    np.full(b, t, dtype=np.float32).view(np.uint8), np.full(b, k, dtype=np.int32).view(np.uint8),
                    np.full(b, p, dtype=np.float32).view(np.uint8)]))
                out = D.ByteBuffer(12 * b)
                q = params.ptr
                state = {'at': 0}

                def logits():
                    state['at'] = (state['at'] + 1) % slots
                    return region.ptr + 4 * state['at'] * b * vocab

                def sample():
                    desc = _C.npm_sample(logits=logits(), pitch=vocab, batch=b, vocab=vocab, temperature=q + 16 * b, top_k=q + 20 * b,
                                         top_p=q + 24 * b, seed=q, draw=q + 8 * b, token=out.ptr, kept=out.ptr + 4 * b, prob=out.ptr + 8 * b)
                    _C.check(lib.npm_sample_rows(C.byref(desc)), 'npm_sample_rows')

                def softmax():
                    _C.check(lib.npm_softmax_fwd(logits(), scratch.ptr, b, vocab, 1.0), 'npm_softmax_fwd')

                times = {sample: [], softmax: []}
                for fn in times:
                    window(fn, 8)
                for _ in range(a.windows):
                    for fn in times:
                        times[fn].append(window(fn, a.calls))
                fmt = lambda ts: f'{min(ts):9.1f} {sorted(ts)[len(ts) // 2]:9.1f} {max(ts):9.1f}'
                ratio = sorted(times[sample])[a.windows // 2] / sorted(times[softmax])[a.windows // 2]
                print(f'{b:>3} {vocab:>7} {name:>13} | {fmt(times[sample]):>30} | {fmt(times[softmax]):>30} | {ratio:>14.2f} | '
                      f'{_C.last_sample_kernel()}', flush=True)


if __name__ == '__main__':
    main()
