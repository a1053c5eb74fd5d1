#!/usr/bin/env python3
"""What gradient accumulation costs (csrc/npm_accum.hip), in one process:

  (a) the fold: npm_accumulate_ranges without the sum against npm_axpy(alpha = 1) on the same buffers, 12.6 M and 200 M elements,
      as 1 range (one call each) and as 64 ranges (two calls of 32 against 64 calls of npm_axpy, which is what ``fold()`` makes of
      them on either route): both read dst and src and write dst -- 12 bytes per element; the yardstick is npm_axpy;
  (b) the norm in the last fold: npm_accumulate_ranges with the sum against npm_accumulate_ranges without it followed by
      npm_sumsq_ranges over dst -- the same bits, 12 against 16 bytes per element; the yardstick is the two calls;
  (c) a training step of ``models.CausalLM`` (d 1024, hidden 2688, 4 layers, vocabulary 32000, global B 8, S 512) through
      ``train.Trainer`` with ``AdamWOptimizer(clip_norm=1.0, accumulate=True)`` at ``micro_batches`` 1, 2 and 4 (2 also with
      device.ACCUM_FUSED_NORM the other way), against ``micro_batches=1`` with ``accumulate=False``, the path of before; and the
      pool's reserved bytes after one call of each from a trimmed pool, which is its peak (the pool keeps what it frees).

Cold buffers: successive calls of (a) and (b) walk through (dst, src) sets that together cover at least --region-mb (four times the
Infinity Cache by default); a set of that size or more is its own cold region.  Microseconds per call from HIP events around a
window of back-to-back calls, launch gaps included; the variants alternate; median (min .. max) over the windows.  A ratio is to be
read beside the yardstick's own spread, printed with it; ``**`` marks a new route that is slower than its yardstick beyond that.

    python tools/accum_bench.py > profiles/r28_accum_bench.log
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='12600000,200000000')
    ap.add_argument('--region-mb', type=int, default=1024)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--window-ms', type=float, default=40.0, help='work per timed window, at least')
    ap.add_argument('--max-calls', type=int, default=32)
    ap.add_argument('--model-steps', type=int, default=4, help='training steps per timed window of (c); 0 skips (c)')
    ap.add_argument('--model-shape', default='32000,1024,2688,4,8,512', help='vocabulary, d, hidden, layers, global B, S of (c)')
    a = ap.parse_args()

    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    print(f'accum_bench: sources {_C.source_id()}; {a.windows} windows of at least {a.window_ms:g} ms per variant, alternating, after untimed '
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

    def ratio(new, yard):
        r = med(new) / med(yard)
        return f'{"**" if r > 1.0 + spread(yard) else ""}{r:.3f}{"**" if r > 1.0 + spread(yard) else ""}'

    def filled(count):
        out = D.empty([count])
        for at in range(0, count, chunk):
            _C.check(lib.npm_d2d(out.ptr + 4 * at, noise.ptr, 4 * min(chunk, count - at)), 'npm_d2d')
        return out

    for n in (int(v) for v in a.sizes.split(',')):
        D.trim_pool()
        slots = max(1, -(-a.region_mb * (1 << 20) // (8 * n)))
        dst, src = filled(slots * n), filled(slots * n)
        acc = D._Buffer(8)
        _C.check(lib.npm_fill_f64(acc.ptr, 0.0, 1), 'npm_fill_f64')
        state = {'at': 0}

        def slot():
            state['at'] = (state['at'] + 1) % slots
            return state['at']

        def cuts(parts):
            per = n // parts
            return [per * i for i in range(parts)] + [n]

        def tables(parts):
            """Per slot: [(dst table, src table), ...], 32 pairs a table."""
            made, edges = [], cuts(parts)
            for s in range(slots):
                d0, s0, each = dst.ptr + 4 * s * n, src.ptr + 4 * s * n, []
                for lo in range(0, parts, _C.SUMSQ_MAX_RANGES):
                    td, ts = _C.npm_ranges(), _C.npm_ranges()
                    for i, p in enumerate(range(lo, min(lo + _C.SUMSQ_MAX_RANGES, parts))):
                        td.ptr[i], ts.ptr[i] = d0 + 4 * edges[p], s0 + 4 * edges[p]
                        td.n[i] = ts.n[i] = edges[p + 1] - edges[p]
                    td.count = ts.count = min(_C.SUMSQ_MAX_RANGES, parts - lo)
                    each.append((td, ts))
                made.append(each)
            return made

        def fold(made, with_sum=False, then_sumsq=False):
            def call():
                each = made[slot()]
                for td, ts in each:
                    _C.check(lib.npm_accumulate_ranges(C.byref(td), C.byref(ts), acc.ptr if with_sum else None), 'npm_accumulate_ranges')
                if then_sumsq:
                    for td, _ in each:
                        _C.check(lib.npm_sumsq_ranges(C.byref(td), acc.ptr), 'npm_sumsq_ranges')
            return call

        def axpy(parts):
            edges = cuts(parts)

            def call():
                at = slot() * n
                for p in range(parts):
                    _C.check(lib.npm_axpy(dst.ptr + 4 * (at + edges[p]), src.ptr + 4 * (at + edges[p]), 1.0, edges[p + 1] - edges[p]), 'npm_axpy')
            return call

        one, many = tables(1), tables(64)
        share = lambda ts, nbytes: nbytes * n / (med(ts) * 1e-6) / PEAK
        # ---- (a) the fold against npm_axpy ------------------------------------------------------------------------------------------
        t_f1, t_a1, t_f64, t_a64 = measure([fold(one), axpy(1), fold(many), axpy(64)])
        print(f'\n(a) {n} elements ({12 * n / 2 ** 20:.0f} MB moved per fold, {slots} cold set{"" if slots == 1 else "s"})', flush=True)
        print(f'  npm_accumulate_ranges, 1 range     {fmt(t_f1)}   {share(t_f1, 12):5.3f} of 8 TB/s')
        print(f'  npm_axpy, 1 call                   {fmt(t_a1)}   {share(t_a1, 12):5.3f} of 8 TB/s')
        print(f'  npm_accumulate_ranges, 64 ranges   {fmt(t_f64)}   {share(t_f64, 12):5.3f} of 8 TB/s   (two calls of 32)')
        print(f'  npm_axpy, 64 calls                 {fmt(t_a64)}   {share(t_a64, 12):5.3f} of 8 TB/s')
        print(f'  1 range: fold / axpy {ratio(t_f1, t_a1)} (spread of axpy: {spread(t_a1):.3f} of its median)   '
              f'64 ranges: fold / axpy {ratio(t_f64, t_a64)} (spread of axpy: {spread(t_a64):.3f})', flush=True)
        # ---- (b) the norm in the last fold against two calls --------------------------------------------------------------------------
        t_u1, t_t1, t_u64, t_t64 = measure([fold(one, with_sum=True), fold(one, then_sumsq=True),
                                            fold(many, with_sum=True), fold(many, then_sumsq=True)])
        print(f'\n(b) {n} elements (fused: {12 * n / 2 ** 20:.0f} MB moved, fold + npm_sumsq_ranges: {16 * n / 2 ** 20:.0f} MB)', flush=True)
        print(f'  fold with the sum, 1 range         {fmt(t_u1)}   {share(t_u1, 12):5.3f} of 8 TB/s')
        print(f'  fold, then npm_sumsq_ranges        {fmt(t_t1)}   {share(t_t1, 16):5.3f} of 8 TB/s')
        print(f'  fold with the sum, 64 ranges       {fmt(t_u64)}   {share(t_u64, 12):5.3f} of 8 TB/s')
        print(f'  fold, then npm_sumsq_ranges        {fmt(t_t64)}   {share(t_t64, 16):5.3f} of 8 TB/s')
        print(f'  1 range: fused / two calls {ratio(t_u1, t_t1)} (spread of the two calls: {spread(t_t1):.3f})   '
              f'64 ranges: fused / two calls {ratio(t_u64, t_t64)} (spread: {spread(t_t64):.3f})', flush=True)
        del dst, src, one, many

    # ---- (c) a training step ----------------------------------------------------------------------------------------------------------
    if a.model_steps > 0:
        import np_modeling_amd as npm
        vocab, feat, hidden, layers, batch, seq = (int(v) for v in a.model_shape.split(','))
        ids = rng.integers(0, vocab, size=[batch, seq + 1])
        inputs, targets = ids[:, :-1].copy(), ids[:, 1:].copy()

        def stepper(k, accumulate, fused=None):
            made = {}

            def call():
                if not made:
                    np.random.seed(1)
                    made['lm'] = npm.models.CausalLM(vocab, feat, layers, 16, hidden)
                    made['opt'] = npm.optimizer.AdamWOptimizer(1e-4, clip_norm=1.0, accumulate=accumulate)
                    loss = npm.loss.SoftmaxCrossEntropyLoss(reduction='sum' if k > 1 else 'mean')
                    made['trainer'] = npm.train.Trainer([made['lm']], loss)
                saved = D.ACCUM_FUSED_NORM
                D.ACCUM_FUSED_NORM = saved if fused is None else fused
                try:
                    with contextlib.redirect_stdout(io.StringIO()):
                        if k == 1 and not accumulate:
                            made['trainer'].train(inputs, targets, a.model_steps, made['opt'])         # the call of before
                        else:
                            made['trainer'].train(inputs, targets, a.model_steps, made['opt'], micro_batches=k)
                finally:
                    D.ACCUM_FUSED_NORM = saved
            call.made = made
            return call

        variants = [('accumulate=False, micro_batches 1 (the path of before)', stepper(1, False)),
                    ('accumulate=True,  micro_batches 1', stepper(1, True)),
                    ('accumulate=True,  micro_batches 2, fused norm on', stepper(2, True, True)),
                    ('accumulate=True,  micro_batches 2, fused norm off', stepper(2, True, False)),
                    ('accumulate=True,  micro_batches 4, fused norm on', stepper(4, True, True)),
                    ('accumulate=True,  micro_batches 4, fused norm off', stepper(4, True, False))]
        peaks = []
        for name, fn in variants:                               # memory first: each variant alone, from a trimmed pool
            D.trim_pool()
            fn()
            D.synchronize()
            peaks.append(D.pool_stats()[1])
            fn.made.clear()
        D.trim_pool()
        times = measure([fn for _, fn in variants], max_calls=3)
        times = [[t / a.model_steps for t in ts] for ts in times]
        print(f'\n(c) CausalLM d {feat} hidden {hidden} layers {layers} vocabulary {vocab} global B {batch} S {seq}, AdamWOptimizer(clip_norm=1.0): '
              f'microseconds per training step (Trainer.train of {a.model_steps} steps per call, its upload of the ids included); ratio to the '
              f'path of before (its spread: {spread(times[0]):.3f} of its median); reserved pool bytes after one call alone', flush=True)
        for (name, fn), ts, peak in zip(variants, times, peaks):
            last = fn.made['opt'].last
            print(f'  {name:56s} {fmt(ts)}   {ratio(ts, times[0]) if ts is not times[0] else "1.000"}   pool {peak / 2 ** 20:8.0f} MB   '
                  f'folds {last["folds"]} fold launches {last["fold_launches"]} fused {last["fused_norm"]} ranges {last["ranges"]}', flush=True)


if __name__ == '__main__':
    main()
