#!/usr/bin/env python3
"""What AdamW with global-norm clipping costs (csrc/npm_clip.hip), in one process:

  (a) npm_adamw_step against npm_adam_step on the same buffers, 12.6 M and 200 M elements: both read the parameter, the gradient
      and two fp64 moments and write the parameter and the moments back -- 44 bytes per element; the yardstick is the older kernel;
  (b) npm_sumsq_ranges over a tensor as one range and as 64 ranges of the same total (two calls of 32) against npm_scale on the
      same tensor: the sum reads 4 bytes per element, the yardstick reads 4 and writes 4; the ratio and the fraction of 8 TB/s;
  (c) a training step of ``models.CausalLM`` (d 1024, hidden 2688, 4 layers, vocabulary 32000, B 8, S 512) through ``train.Trainer``
      with ``AdamOptimizer`` against ``AdamWOptimizer(clip_norm=1.0)``.

Cold buffers: successive calls of (a) and (b) walk through copies that together cover at least --region-mb (four times the
Infinity Cache by default); a set of that size or more is its own cold region.  Microseconds per call from HIP events around a
window of back-to-back calls, launch gaps included; the variants alternate; median (min .. max) over the windows.

    python tools/adamw_bench.py > profiles/adamw_bench.log
"""
import argparse
import contextlib
import ctypes as C
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8e12
HYPER = (1e-3, 0.9, 0.999, 1e-8)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='12600000,200000000')
    ap.add_argument('--region-mb', type=int, default=1024)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-ms', type=float, default=40.0, help='work per timed window, at least')
    ap.add_argument('--max-calls', type=int, default=32)
    ap.add_argument('--model-steps', type=int, default=4, help='training steps per timed window of (c); 0 skips (c)')
    a = ap.parse_args()

    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    print(f'adamw_bench: sources {_C.source_id()}; {a.windows} windows of at least {a.window_ms:g} ms per variant, alternating, after untimed '
          f'calls; buffers walk a region of at least {a.region_mb} MB; microseconds per call, median (min .. max)', flush=True)
    rng = np.random.default_rng(0)
    chunk = 1 << 22
    noise = D.from_host(rng.standard_normal(chunk).astype(np.float32))

    def window(fn, calls):
        start = D.Event().record()
        for _ in range(calls):
            fn()
        stop = D.Event().record()
        stop.synchronize()
        return start.elapsed_ms(stop) * 1e3 / calls

    def measure(fns, max_calls=None):
        calls = {}
        for fn in fns:
            fn()                                                # code objects, first touch
            once = window(fn, 2)
            calls[fn] = int(min(max_calls or a.max_calls, max(3, a.window_ms * 1e3 / max(once, 1.0))))
        times = {fn: [] for fn in fns}
        for _ in range(a.windows):
            for fn in fns:
                times[fn].append(window(fn, calls[fn]))
        return [times[fn] for fn in fns]

    med = lambda ts: sorted(ts)[len(ts) // 2]
    fmt = lambda ts: f'{med(ts):10.1f} ({min(ts):.1f} .. {max(ts):.1f})'
    spread = lambda ts: (max(ts) - min(ts)) / med(ts)

    def filled(count):
        out = D.empty([count])
        for at in range(0, count, chunk):
            _C.check(lib.npm_d2d(out.ptr + 4 * at, noise.ptr, 4 * min(chunk, count - at)), 'npm_d2d')
        return out

    for n in (int(v) for v in a.sizes.split(',')):
        # ---- (a) the step: slots of (parameter, gradient, two moments) -----------------------------------------------------------
        D.trim_pool()
        slots = max(1, -(-a.region_mb * (1 << 20) // (24 * n)))
        var, grad = filled(slots * n), filled(slots * n)
        first, second = D._Buffer(8 * slots * n), D._Buffer(8 * slots * n)
        for buf in (first, second):
            _C.check(lib.npm_fill_f64(buf.ptr, 0.0, slots * n), 'npm_fill_f64')
        state = {'at': 0}

        def slot():
            state['at'] = (state['at'] + 1) % slots
            return state['at'] * n

        def adam():
            at = slot()
            _C.check(lib.npm_adam_step(var.ptr + 4 * at, grad.ptr + 4 * at, first.ptr + 8 * at, second.ptr + 8 * at, n, *HYPER, 10), 'npm_adam_step')

        clip = D._Buffer(32)
        _C.check(lib.npm_h2d(clip.ptr, np.array([4.0, 2.0, 0.5, 1.0]).ctypes.data, 32), 'npm_h2d')

        def adamw(state_ptr):
            def call():
                at = slot()
                _C.check(lib.npm_adamw_step(var.ptr + 4 * at, grad.ptr + 4 * at, first.ptr + 8 * at, second.ptr + 8 * at, n, *HYPER, 10, 0.1,
                                            state_ptr), 'npm_adamw_step')
            return call

        plain, clipped = adamw(None), adamw(clip.ptr)
        t_adam, t_plain, t_clipped = measure([adam, plain, clipped])
        share = lambda ts, nbytes: nbytes * n / (med(ts) * 1e-6) / PEAK
        print(f'\n(a) {n} elements ({44 * n / 2 ** 20:.0f} MB moved per call, {slots} cold set{"" if slots == 1 else "s"})', flush=True)
        print(f'  npm_adam_step                  {fmt(t_adam)}   {share(t_adam, 44):5.3f} of 8 TB/s')
        print(f'  npm_adamw_step, clip NULL      {fmt(t_plain)}   {share(t_plain, 44):5.3f} of 8 TB/s')
        print(f'  npm_adamw_step, clip state     {fmt(t_clipped)}   {share(t_clipped, 44):5.3f} of 8 TB/s')
        print(f'  adamw / adam {med(t_plain) / med(t_adam):6.3f}   adamw with clip state / adam {med(t_clipped) / med(t_adam):6.3f}   '
              f'(spread of adam: {spread(t_adam):.3f} of its median)', flush=True)
        del var, grad, first, second

        # ---- (b) the sum of squares -----------------------------------------------------------------------------------------------
        D.trim_pool()
        slots = max(1, -(-a.region_mb * (1 << 20) // (4 * n)))
        region, out = filled(slots * n), D.empty([n])
        acc = D._Buffer(8)
        _C.check(lib.npm_fill_f64(acc.ptr, 0.0, 1), 'npm_fill_f64')
        state['at'] = 0

        def tables(parts):
            made = []
            for s in range(slots):
                base, per, each = region.ptr + 4 * s * n, n // parts, []
                cuts = [per * i for i in range(parts)] + [n]
                for lo in range(0, parts, _C.SUMSQ_MAX_RANGES):
                    table = _C.npm_ranges()
                    for i, p in enumerate(range(lo, min(lo + _C.SUMSQ_MAX_RANGES, parts))):
                        table.ptr[i], table.n[i] = base + 4 * cuts[p], cuts[p + 1] - cuts[p]
                    table.count = min(_C.SUMSQ_MAX_RANGES, parts - lo)
                    each.append(table)
                made.append(each)
            return made

        def sumsq(made):
            def call():
                for table in made[slot() // n]:
                    _C.check(lib.npm_sumsq_ranges(C.byref(table), acc.ptr), 'npm_sumsq_ranges')
            return call

        def scale():
            _C.check(lib.npm_scale(region.ptr + 4 * slot(), out.ptr, 0.5, n), 'npm_scale')

        one, many = sumsq(tables(1)), sumsq(tables(64))
        t_one, t_many, t_scale = measure([one, many, scale])
        print(f'\n(b) {n} elements ({4 * n / 2 ** 20:.0f} MB read, {slots} cold cop{"y" if slots == 1 else "ies"})', flush=True)
        print(f'  npm_sumsq_ranges, 1 range      {fmt(t_one)}   {share(t_one, 4):5.3f} of 8 TB/s')
        print(f'  npm_sumsq_ranges, 64 ranges    {fmt(t_many)}   {share(t_many, 4):5.3f} of 8 TB/s   (two calls of 32)')
        print(f'  npm_scale (1 read, 1 write)    {fmt(t_scale)}   {share(t_scale, 8):5.3f} of 8 TB/s')
        print(f'  1 range / npm_scale {med(t_one) / med(t_scale):6.3f}   64 ranges / npm_scale {med(t_many) / med(t_scale):6.3f}   '
              f'(spread of npm_scale: {spread(t_scale):.3f} of its median)', flush=True)
        del region, out

    # ---- (c) a training step ------------------------------------------------------------------------------------------------------
    if a.model_steps > 0:
        import np_modeling_amd as npm
        D.trim_pool()
        vocab, feat, hidden, layers, batch, seq = 32000, 1024, 2688, 4, 8, 512
        ids = rng.integers(0, vocab, size=[batch, seq + 1])
        inputs, targets = ids[:, :-1].copy(), ids[:, 1:].copy()

        def stepper(optimizer):
            np.random.seed(1)
            lm = npm.models.CausalLM(vocab, feat, layers, 16, hidden)
            trainer = npm.train.Trainer([lm], npm.loss.SoftmaxCrossEntropyLoss())

            def call():
                with contextlib.redirect_stdout(io.StringIO()):
                    trainer.train(inputs, targets, a.model_steps, optimizer)
            return call

        adam_opt, adamw_opt = npm.optimizer.AdamOptimizer(1e-4), npm.optimizer.AdamWOptimizer(1e-4, clip_norm=1.0)
        t_adam, t_adamw = measure([stepper(adam_opt), stepper(adamw_opt)], max_calls=3)
        per = lambda ts: [t / a.model_steps for t in ts]
        t_adam, t_adamw = per(t_adam), per(t_adamw)
        norm, factor, ok = adamw_opt.last_grad_norm()
        print(f'\n(c) CausalLM d {feat} hidden {hidden} layers {layers} vocabulary {vocab} B {batch} S {seq}: microseconds per training step '
              f'(Trainer.train of {a.model_steps} steps per call, its upload of the ids included)', flush=True)
        print(f'  AdamOptimizer                  {fmt(t_adam)}')
        print(f'  AdamWOptimizer(clip_norm=1.0)  {fmt(t_adamw)}   launches {adamw_opt.last["launches"]} updates {adamw_opt.last["updates"]} '
              f'ranges {adamw_opt.last["ranges"]}; last norm {norm:.4g} factor {factor:.4g} ok {ok}')
        print(f'  adamw / adam {med(t_adamw) / med(t_adam):6.3f}   (spread of adam: {spread(t_adam):.3f} of its median)', flush=True)


if __name__ == '__main__':
    main()
