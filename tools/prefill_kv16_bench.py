#!/usr/bin/env python3
"""What the fp16 instance of the prefill attention kernel (npm_mha_prefill_fwd_f16, csrc/npm_prefill.hip) buys the cached forwards
over a half-precision cache that the decode kernel does not take, on the cases of tools/prefill_bench.py: D 128, Hq 8, Hkv in
{8, 1}, page size 64.  Timed is the ATTENTION PART of ``att(x, cache=cache, ...)`` -- the layer's own ``_attend`` on a cache that
already holds this call's rows -- end to end by WALL CLOCK around a device synchronisation, so the switch-off path pays what it really pays per call: gathering K / V into fp32 copies, building the mask with NumPy, uploading
it, its tile summary, and the fused forward.  The arms of a case run in one process, interleaved, after one untimed call each:
the switch-off arm first and the kernel arms behind it in rotating order, so that each of them follows the switch-off arm (and the
frees of its gathered copies) equally often.  K / V are cold (512 MB are written between two timed calls, twice the Infinity
Cache); min / median / max, and the median of the part of it the host spends before everything is enqueued:

  f16 off    an fp16 cache, ``device.PREFILL_KERNEL_F16`` off: gather + mask + fused forward (what every call was)
  f16 on     the same cache, the switch on: npm_mha_prefill_fwd_f16 over the stored halves in place
  f32 on     an fp32 cache holding the same rows, ``device.PREFILL_KERNEL`` on: npm_mha_prefill_fwd -- the same kernel body at the
  f32 on'    same shape; run as two series, so that their difference shows the run-to-run spread
  f16 kern   case (c) only: npm_mha_prefill_fwd_f16 called as the fp32 arms of that case are called (see there)

  (a) admission     B 64, one slot brings 512 tokens, the others 1 (T = 512 padded), lengths uniform in 1 .. 8192 (seeded), paged
  (b) chunk         B 8, T = 512 onto 2048 cached rows, paged
  (c) from empty    B 8, T = 2048, contiguous and uniform: an fp16 cache is attended to as stored, so the switch does send this
                    case to the kernel.  The layer sends an fp32 cache of this case to the fused forward, so the fp32 arms call
                    ``cache.attend(kernel='prefill')`` themselves, as tools/prefill_bench.py does; a fifth arm, ``f16 kern``, makes
                    the same direct call on the fp16 cache, and the kernel-against-kernel line of this case compares those

Also: the bytes the pool newly reserves for one call after a trim, per arm (the gathered fp32 copies, the mask and its summary,
against q-sized outputs).

    python tools/prefill_kv16_bench.py > profiles/r15_prefill_kv16_bench.log
"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FLUSH_FLOATS = 128 << 20          # 512 MB


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--kv', default='8,1')
    ap.add_argument('--h', type=int, default=8)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--page', type=int, default=64)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--budget-s', type=float, default=12.0, help='stop repeating a case after this long (at least 3 repetitions)')
    ap.add_argument('--only', default='', help='cases to run, e.g. a or b,c')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--shrink', type=int, default=1, help='divide batch, tokens and lengths by this (a rehearsal, not a measurement)')
    a = ap.parse_args()

    import np_modeling_amd as npm
    from np_modeling_amd import _C, device as D
    from np_modeling_amd.device import Mat
    h, d, page = a.h, a.d, a.page
    f = h * d
    scale = 1.0 / math.sqrt(d)
    only = [c for c in a.only.split(',') if c]
    sh = max(a.shrink, 1)
    flush = D.empty([FLUSH_FLOATS // sh ** 2])
    print(f'prefill_kv16_bench: sources {_C.source_id()}, Hq {h} D {d} page {page}; wall clock around a sync, {a.reps} repetitions per arm '
          f'(interleaved) after one untimed call each, {4 * flush.size >> 20} MB written before every timed call; milliseconds per call'
          + (f'; SHRUNK by {sh}: a rehearsal, not a measurement' if sh > 1 else ''), flush=True)

    def timed(fn):
        _C.check(_C.lib().npm_fill_f32(flush.ptr, 0.0, flush.size), 'npm_fill_f32')       # K / V leave the caches
        D.synchronize()
        t0 = time.perf_counter()
        out = fn()
        th = time.perf_counter()                                          # the host is done: everything is enqueued
        D.synchronize()
        t1 = time.perf_counter()
        del out
        return (t1 - t0) * 1e3, (th - t0) * 1e3

    def compare(tag, arms, kernel_arm='f16 on'):
        """arms: [(name, what, () -> ctx)]; ``kernel_arm`` is the fp16 arm called at the level of the fp32 arms.  Returns {name: median}."""
        grow = {}
        for name, _, fn in arms:
            D.synchronize()
            D.trim_pool()
            before = D.pool_stats()[1]
            timed(fn)                                                     # untimed: first-use allocations
            grow[name] = D.pool_stats()[1] - before
        t, host = {name: [] for name, _, _ in arms}, {name: [] for name, _, _ in arms}
        start = time.perf_counter()
        for rep in range(a.reps):
            turn = rep % (len(arms) - 1)                                  # the kernel arms follow the switch-off arm in turn
            for name, _, fn in arms[:1] + arms[1 + turn:] + arms[1:1 + turn]:
                total, enqueue = timed(fn)
                t[name].append(total)
                host[name].append(enqueue)
            if rep >= 2 and time.perf_counter() - start > a.budget_s:
                break
        stats = {k: (min(v), sorted(v)[len(v) // 2], max(v)) for k, v in t.items()}
        for name, what, _ in arms:
            s = stats[name]
            print(f'{tag:<36} {name:<8} {what:<40} {s[0]:10.2f} {s[1]:10.2f} {s[2]:10.2f}   host {sorted(host[name])[len(host[name]) // 2]:7.3f}   '
                  f'pool +{grow[name] / 2 ** 20:9.1f} MB   ({len(t[name])} reps)', flush=True)
        med = {k: s[1] for k, s in stats.items()}
        spread = abs(med['f32 on'] - med["f32 on'"])
        print(f'{tag:<36} f16 on / f16 off (medians) {med["f16 on"] / med["f16 off"]:.4f} = {med["f16 off"] / med["f16 on"]:.1f} x; '
              f'pool {grow["f16 on"] / 2 ** 20:.1f} / {grow["f16 off"] / 2 ** 20:.1f} MB', flush=True)
        slower = med[kernel_arm] - min(med['f32 on'], med["f32 on'"])
        print(f'{tag:<36} {kernel_arm} - f32 on (medians) {slower:+.3f} ms; the two f32 series differ by {spread:.3f} ms: '
              f'{"SLOWER beyond the spread" if slower > spread else "faster beyond the spread" if -slower > spread else "within the spread"}', flush=True)
        return med

    def fill(caches, rows, hkv, rng):
        """``rows`` [B] cache rows per sequence, 512 at a time out of one random chunk -- the same rows into every cache."""
        b = len(rows)
        step = 512 // sh
        src = D.from_host(rng.standard_normal([b, step, hkv * d]).astype(np.float32))
        for cache in caches:
            for first in range(0, int(rows.max()), step):
                n = np.clip(rows - first, 0, step)
                cache.append(Mat(src, hkv * d), Mat(src, hkv * d), step, new_lengths=n)
            assert cache.lengths.tolist() == rows.tolist()

    def setting(name, value, fn):
        def run():
            setattr(D, name, value)
            try:
                return fn()
            finally:
                setattr(D, name, False)
        return run

    def arms(call, half, full, what_off, what16, what32):
        """``call(cache)``: () -> ctx over that cache, through the layer."""
        return [('f16 off', what_off, setting('PREFILL_KERNEL_F16', False, call(half))),
                ('f16 on', what16, setting('PREFILL_KERNEL_F16', True, call(half))),
                ('f32 on', what32, setting('PREFILL_KERNEL', True, call(full))),
                ("f32 on'", what32, setting('PREFILL_KERNEL', True, call(full)))]

    for hkv in (int(x) for x in a.kv.split(',')):
        att = npm.layers.MultiHeadAttention(h, num_kv_heads=hkv)
        np.random.seed(0)
        att(np.zeros([1, 2, f], dtype=np.float32))
        rng = np.random.default_rng(a.seed)
        print(f'Hkv {hkv}:{"":>84} min     median        max   host: median ms until everything is enqueued', flush=True)

        if not only or 'a' in only:
            b, t, lmax = max(64 // sh, 2), 512 // sh, 8192 // sh
            lengths = rng.integers(1, lmax + 1, b)
            lengths[0] = max(int(lengths[0]), t)
            n = np.array([t] + [1] * (b - 1), dtype=np.int64)
            pages = int(np.sum(-(-lengths // page)))
            half = D.PagedKVCache(b, lmax, hkv, d, page_size=page, pages=pages, dtype='f16')
            full = D.PagedKVCache(b, lmax, hkv, d, page_size=page, pages=pages)
            fill((half, full), lengths, hkv, rng)
            q = D.from_host(rng.standard_normal([b, t, h, d]).astype(np.float32))
            before = half.lengths - n
            call = lambda cache: lambda: att._attend(Mat(q, f), cache, t, True, None, before, n, True)
            print(f'(a) lengths sum {int(lengths.sum())} = {lengths.sum() / (b * lmax):.3f} B Lmax, max {int(lengths.max())}; the caches hold '
                  f'{half.nbytes / 2 ** 20:.0f} MB (fp16) and {full.nbytes / 2 ** 20:.0f} MB (fp32) of pages; one gathered fp32 K + V = '
                  f'{2 * b * int(lengths.max()) * hkv * d * 4 / 2 ** 20:.0f} MB', flush=True)
            compare(f'(a) admission B {b} T {t} Hkv {hkv}', arms(call, half, full, 'gather_f16 + mask + fused forward',
                                                                 'npm_mha_prefill_fwd_f16 paged', 'npm_mha_prefill_fwd paged'))
            assert att._cached_path == 'prefill'
            del half, full, q
            D.trim_pool()

        if not only or 'b' in only:
            b, t, have = max(8 // sh, 2), 512 // sh, 2048 // sh
            rows = np.full(b, have + t)
            n = np.full(b, t, dtype=np.int64)
            q = D.from_host(rng.standard_normal([b, t, h, d]).astype(np.float32))
            half = D.PagedKVCache(b, have + t, hkv, d, page_size=page, dtype='f16')
            full = D.PagedKVCache(b, have + t, hkv, d, page_size=page)
            fill((half, full), rows, hkv, rng)
            call = lambda cache: lambda: att._attend(Mat(q, f), cache, t, True, None, rows - n, None, True)
            compare(f'(b) chunk B {b} T {t} on {have} paged', arms(call, half, full, 'gather_f16 + mask + fused forward',
                                                                   'npm_mha_prefill_fwd_f16 paged', 'npm_mha_prefill_fwd paged'))
            assert att._cached_path == 'prefill'
            del half, full, q
            D.trim_pool()

        if not only or 'c' in only:
            b, t = max(8 // sh, 2), 2048 // sh
            q = D.from_host(rng.standard_normal([b, t, h, d]).astype(np.float32))
            half, full = D.KVCache(b, t, hkv, d, dtype='f16'), D.KVCache(b, t, hkv, d)
            fill((half, full), np.full(b, t), hkv, rng)
            through_layer = lambda cache: lambda: att._attend(Mat(q, f), cache, t, True, None, cache.lengths - t, None, False)
            forced = lambda cache: lambda: cache.attend(Mat(q, f), h, t, scale, True, kernel='prefill')[0]
            compare(f'(c) from empty B {b} T {t} Hkv {hkv}',
                    [('f16 off', 'gather_f16 + mask + fused forward', setting('PREFILL_KERNEL_F16', False, through_layer(half))),
                     ('f16 on', 'npm_mha_prefill_fwd_f16', setting('PREFILL_KERNEL_F16', True, through_layer(half))),
                     ('f16 kern', 'npm_mha_prefill_fwd_f16 (direct)', setting('PREFILL_KERNEL_F16', True, forced(half))),
                     ('f32 on', 'npm_mha_prefill_fwd (direct)', forced(full)), ("f32 on'", 'npm_mha_prefill_fwd (direct)', forced(full))],
                    kernel_arm='f16 kern')
            assert att._cached_path == 'prefill'
            del half, full, q
            D.trim_pool()
        print(f'last prefill kernel: {_C.last_prefill_kernel()}', flush=True)


if __name__ == '__main__':
    main()
