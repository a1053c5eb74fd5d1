#!/usr/bin/env python3
"""What softmax cross-entropy from logits costs (npm_softmax_xent_rows), in one process, per shape rows x V:

  * the new call: loss only, loss + gradient into a second tensor, loss + gradient in place;
  * what a user had to run before, on the same logits: npm_softmax_fwd + npm_xent_fwd + npm_xent_bwd + npm_softmax_bwd against a dense
    one-hot [rows, V] float tensor (three more [rows, V] tensors: the probabilities, -t / y and the gradient);
  * npm_scale over the same [rows, V]: one read and one write of every element, the bandwidth yardstick of the gradient call.

Cold rows: successive calls walk through copies of the logits that together cover at least 1 GB (four times the Infinity Cache); a
tensor of 1 GB or more is its own cold region.  Microseconds per call from HIP events around a window of back-to-back calls, launch
gaps and the call's own 8-byte copy to the host included; the variants alternate; median (min .. max) over the windows.  The
in-place variant turns logits into gradients, so later windows read those: the work does not depend on the values.  "of 8 TB/s":
the bytes the call must move (4 V per row read, 4 V more written with a gradient) over the median time, as a fraction of the HBM
peak.  "reserved": the pool's reserved bytes (npm_pool_stats) while the variant's buffers are alive, the logits included.

    python tools/xent_bench.py > profiles/r22_xent_bench.log
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = '512x32000,4096x32000,16384x32000,512x128256,4096x128256,16384x128256,65536x512'
PEAK = 8e12


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default=SHAPES)
    ap.add_argument('--region-mb', type=int, default=1024)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-ms', type=float, default=60.0, help='work per timed window, at least')
    ap.add_argument('--max-calls', type=int, default=32)
    a = ap.parse_args()

    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    print(f'xent_bench: sources {_C.source_id()}; {a.windows} windows of at least {a.window_ms:g} ms per variant, alternating, after untimed '
          f'calls; logits walk a region of at least {a.region_mb} MB; microseconds per call, median (min .. max)', flush=True)
    rng = np.random.default_rng(0)
    chunk = 1 << 22
    noise = D.from_host((4 * rng.standard_normal(chunk)).astype(np.float32))

    def window(fn, calls):
        start = D.Event().record()
        for _ in range(calls):
            fn()
        stop = D.Event().record()
        stop.synchronize()
        return start.elapsed_ms(stop) * 1e3 / calls

    def measure(fns):
        calls = {}
        for fn in fns:
            fn()                                                # code objects, first touch
            once = window(fn, 2)
            calls[fn] = int(min(a.max_calls, max(3, a.window_ms * 1e3 / max(once, 1.0))))
        times = {fn: [] for fn in fns}
        for _ in range(a.windows):
            for fn in fns:
                times[fn].append(window(fn, calls[fn]))
        return [times[fn] for fn in fns]

    med = lambda ts: sorted(ts)[len(ts) // 2]
    fmt = lambda ts: f'{med(ts):10.1f} ({min(ts):.1f} .. {max(ts):.1f})'
    reserved = lambda: D.pool_stats()[1]

    for shape in a.shapes.split(','):
        rows, vocab = (int(v) for v in shape.split('x'))
        n = rows * vocab
        slots = max(1, -(-a.region_mb * (1 << 20) // (4 * n)))
        D.trim_pool()
        region = D.empty([slots * n])
        for at in range(0, slots * n, chunk):
            _C.check(lib.npm_d2d(region.ptr + 4 * at, noise.ptr, 4 * min(chunk, slots * n - at)), 'npm_d2d')
        targets = rng.integers(0, vocab, size=rows)
        ids = D.ids_from_host(targets)
        per_row = D.empty([2, rows])
        total = C.c_double()
        state = {'at': 0}

        def logits():
            state['at'] = (state['at'] + 1) % slots
            return region.ptr + 4 * state['at'] * n

        def xent(grad_of):
            def call():
                z = logits()
                _C.check(lib.npm_softmax_xent_rows(z, vocab, ids.ptr, rows, vocab, 0.0, 1.0 / rows, grad_of(z), vocab, per_row.ptr,
                                                   per_row.ptr + 4 * rows, C.byref(total)), 'npm_softmax_xent_rows')
            return call

        base = reserved()
        loss_only, in_place = xent(lambda z: None), xent(lambda z: z)
        t_loss, = measure([loss_only])
        loss_kernel, r_loss = _C.last_xent_kernel(), reserved()

        grad = D.empty([rows, vocab])
        fresh = xent(lambda z: grad.ptr)

        def scale():
            _C.check(lib.npm_scale(logits(), grad.ptr, 0.5, n), 'npm_scale')

        t_fresh, t_scale = measure([fresh, scale])
        r_fresh = reserved()
        fresh()
        kernel = _C.last_xent_kernel()

        # the composition: a dense one-hot, the probabilities, -t / y; the gradient goes where the new call's went
        one_hot, probs, dprobs = D.empty([rows, vocab]), D.empty([rows, vocab]), D.empty([rows, vocab])
        step = max(1, (1 << 27) // vocab)
        for at in range(0, rows, step):
            block = np.zeros([min(step, rows - at), vocab], dtype=np.float32)
            block[np.arange(block.shape[0]), targets[at:at + step]] = 1.0
            _C.check(lib.npm_h2d(one_hot.ptr + 4 * at * vocab, block.ctypes.data, block.nbytes), 'npm_h2d')

        def composition():
            z = logits()
            _C.check(lib.npm_softmax_fwd(z, probs.ptr, rows, vocab, 1.0), 'npm_softmax_fwd')
            _C.check(lib.npm_xent_fwd(probs.ptr, one_hot.ptr, n, C.byref(total)), 'npm_xent_fwd')
            _C.check(lib.npm_xent_bwd(probs.ptr, one_hot.ptr, dprobs.ptr, n), 'npm_xent_bwd')
            _C.check(lib.npm_softmax_bwd(probs.ptr, dprobs.ptr, grad.ptr, rows, vocab, 1.0), 'npm_softmax_bwd')

        t_old, = measure([composition])
        r_old = reserved()
        del one_hot, probs, dprobs, grad                         # in place needs none of them: back to the logits alone
        D.trim_pool()
        t_in_place, = measure([in_place])
        r_in_place = reserved()

        gb = lambda b: f'{b / 2 ** 30:7.2f} GiB'
        share = lambda ts, passes: 4.0 * n * passes / (med(ts) * 1e-6) / PEAK
        print(f'\n{rows} x {vocab} ({4 * n / 2 ** 20:.0f} MB of logits, {slots} cold cop{"y" if slots == 1 else "ies"}; {kernel}; loss only: '
              f'{loss_kernel.split()[0]})', flush=True)
        print(f'  loss only                     {fmt(t_loss)}   {share(t_loss, 1):5.3f} of 8 TB/s   reserved {gb(r_loss)}')
        print(f'  loss + gradient               {fmt(t_fresh)}   {share(t_fresh, 2):5.3f} of 8 TB/s   reserved {gb(r_fresh)}')
        print(f'  loss + gradient, in place     {fmt(t_in_place)}   {share(t_in_place, 2):5.3f} of 8 TB/s   reserved {gb(r_in_place)}')
        print(f'  npm_scale (1 read, 1 write)   {fmt(t_scale)}   {share(t_scale, 2):5.3f} of 8 TB/s')
        print(f'  softmax + one-hot xent (4)    {fmt(t_old)}                     reserved {gb(r_old)}')
        print(f'  loss + gradient / npm_scale {med(t_fresh) / med(t_scale):6.2f}   in place / npm_scale {med(t_in_place) / med(t_scale):6.2f}   '
              f'composition / loss + gradient {med(t_old) / med(t_fresh):6.2f}   composition / in place {med(t_old) / med(t_in_place):6.2f}   '
              f'(the logits alone: reserved {gb(base)})', flush=True)
        del region


if __name__ == '__main__':
    main()
