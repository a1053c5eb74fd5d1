#!/usr/bin/env python3
"""What the prefill attention kernel (npm_mha_prefill_fwd, csrc/npm_prefill.hip) buys the cached forwards that the decode kernel
does not take, at D 128, Hq 8, Hkv in {8, 1}, page size 64.  Timed is the ATTENTION PART of ``att(x, cache=cache, ...)`` -- the
layer's own ``_attend`` on a cache that already holds this call's rows -- end to end by WALL CLOCK
around a device synchronisation, so the switch-off path pays what it really pays per call: gathering K / V, building the mask with
NumPy, uploading it, its tile summary, and the fused forward.  Both settings of ``device.PREFILL_KERNEL`` run in the same process on
the same cache, interleaved (off, on, off, on, ...), after one untimed call each; min / median / max over the repetitions.

  (a) admission     B 64, one slot brings 512 tokens, the others 1 (T = 512 padded), lengths uniform in 1 .. 8192 (seeded), paged
  (b) chunk         B 8, T = 512 onto 2048 cached rows, paged; and the same on a contiguous cache (a copy per sequence, a T x L mask)
  (c) from empty    B 8, T = 2048, contiguous: the fused forward on the fresh projection (what the layer keeps doing) against the
                    prefill kernel FORCED onto that case -- it informs a later default, the switch does not send this case there

Also: the bytes the pool newly reserves for one call after a trim (the gathered copies, the mask and its summary, against q-sized
outputs), per setting.

    python tools/prefill_bench.py > profiles/r13_prefill_bench.log
"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--kv', default='8,1')
    ap.add_argument('--h', type=int, default=8)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--page', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--budget-s', type=float, default=12.0, help='stop repeating a case after this long (at least 3 repetitions)')
    ap.add_argument('--only', default='', help='cases to run, e.g. a or b,c')
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()

    import np_modeling_amd as npm
    from np_modeling_amd import _C, device as D
    from np_modeling_amd.device import Mat
    h, d, page = a.h, a.d, a.page
    f = h * d
    scale = 1.0 / math.sqrt(d)
    only = [c for c in a.only.split(',') if c]
    print(f'prefill_bench: sources {_C.source_id()}, Hq {h} D {d} page {page}; wall clock around a sync, {a.reps} repetitions per setting '
          f'(interleaved) after one untimed call each; milliseconds per call', flush=True)

    def timed(fn):
        D.synchronize()
        t0 = time.perf_counter()
        out = fn()
        D.synchronize()
        t1 = time.perf_counter()
        del out
        return (t1 - t0) * 1e3

    def compare(tag, off, on, what_off, what_on):
        """off / on: () -> ctx.  Sets nothing itself: the callers flip the switch inside."""
        grow = {}
        for name, fn in (('off', off), ('on', on)):
            D.synchronize()
            D.trim_pool()
            before = D.pool_stats()[1]
            timed(fn)                                                     # untimed: first-use allocations
            grow[name] = D.pool_stats()[1] - before
        t = {'off': [], 'on': []}
        start = time.perf_counter()
        for rep in range(a.reps):
            t['off'].append(timed(off))
            t['on'].append(timed(on))
            if rep >= 2 and time.perf_counter() - start > a.budget_s:
                break
        stats = {k: (min(v), sorted(v)[len(v) // 2], max(v)) for k, v in t.items()}
        for name, what in (('off', what_off), ('on', what_on)):
            s = stats[name]
            print(f'{tag:<34} {name:<3} {what:<34} {s[0]:10.2f} {s[1]:10.2f} {s[2]:10.2f}   pool +{grow[name] / 2 ** 20:9.1f} MB   ({len(t[name])} reps)',
                  flush=True)
        print(f'{tag:<34} on / off (medians) {stats["on"][1] / stats["off"][1]:.4f}   = {stats["off"][1] / stats["on"][1]:.1f} x', flush=True)

    def fill(cache, rows, hkv, rng):
        """``rows`` [B] cache rows per sequence, 512 at a time out of one random chunk."""
        b = len(rows)
        src = D.from_host(rng.standard_normal([b, 512, hkv * d]).astype(np.float32))
        for first in range(0, int(rows.max()), 512):
            n = np.clip(rows - first, 0, 512)
            cache.append(Mat(src, hkv * d), Mat(src, hkv * d), 512, new_lengths=n)
        assert cache.lengths.tolist() == rows.tolist()

    def setting(value, fn):
        def run():
            D.PREFILL_KERNEL = value
            try:
                return fn()
            finally:
                D.PREFILL_KERNEL = False
        return run

    for hkv in (int(x) for x in a.kv.split(',')):
        att = npm.layers.MultiHeadAttention(h, num_kv_heads=hkv)
        np.random.seed(0)
        att(np.zeros([1, 2, f], dtype=np.float32))
        rng = np.random.default_rng(a.seed)
        print(f'Hkv {hkv}:{"":>70} min     median        max', flush=True)

        if not only or 'a' in only:
            b, t, lmax = 64, 512, 8192
            lengths = rng.integers(1, lmax + 1, b)
            lengths[0] = max(int(lengths[0]), t)
            n = np.array([t] + [1] * (b - 1), dtype=np.int64)
            cache = D.PagedKVCache(b, lmax, hkv, d, page_size=page, pages=int(np.sum(-(-lengths // page))))
            fill(cache, lengths, hkv, rng)
            q = D.from_host(rng.standard_normal([b, t, h, d]).astype(np.float32))
            before = cache.lengths - n
            fn = lambda: att._attend(Mat(q, f), cache, t, True, None, before, n, True)
            held = 2 * cache.pages * page * hkv * d * 4 / 2 ** 20
            print(f'(a) lengths sum {int(lengths.sum())} = {lengths.sum() / (b * lmax):.3f} B Lmax, max {int(lengths.max())}; the cache holds {held:.0f} MB of pages; '
                  f'mask [B, 1, T, keys] = {b * t * int(lengths.max()) / 2 ** 20:.0f} MB', flush=True)
            compare(f'(a) admission B {b} T {t} Hkv {hkv}', setting(False, fn), setting(True, fn), 'gather + mask + fused forward', 'npm_mha_prefill_fwd paged')
            assert att._cached_path == 'prefill'
            del cache, q
            D.trim_pool()

        if not only or 'b' in only:
            b, t, have = 8, 512, 2048
            rows = np.full(b, have + t)
            n = np.full(b, t, dtype=np.int64)
            q = D.from_host(rng.standard_normal([b, t, h, d]).astype(np.float32))
            cache = D.PagedKVCache(b, have + t, hkv, d, page_size=page)
            fill(cache, rows, hkv, rng)
            fn = lambda: att._attend(Mat(q, f), cache, t, True, None, rows - n, None, True)
            compare(f'(b) chunk B {b} T {t} on {have} paged', setting(False, fn), setting(True, fn), 'gather + mask + fused forward', 'npm_mha_prefill_fwd paged')
            del cache
            cache = D.KVCache(b, have + t + 64, hkv, d)                   # not full: the fused path copies the valid rows
            fill(cache, rows, hkv, rng)
            fn = lambda: att._attend(Mat(q, f), cache, t, True, None, cache.lengths - t, None, False)
            compare(f'(b) chunk B {b} T {t} on {have} contig.', setting(False, fn), setting(True, fn), 'copy + mask + fused forward', 'npm_mha_prefill_fwd')
            assert att._cached_path == 'prefill'
            del cache, q
            D.trim_pool()

        if not only or 'c' in only:
            b, t = 8, 2048
            q = D.from_host(rng.standard_normal([b, t, h, d]).astype(np.float32))
            fresh = D.from_host(rng.standard_normal([b, t, hkv * d]).astype(np.float32))
            cache = D.KVCache(b, t, hkv, d)
            cache.append(Mat(fresh, hkv * d), Mat(fresh, hkv * d), t)
            off = lambda: att._attend(Mat(q, f), cache, t, True, (Mat(fresh, hkv * d), Mat(fresh, hkv * d)), cache.lengths - t, None, False)
            on = lambda: cache.attend(Mat(q, f), h, t, scale, True, kernel='prefill')[0]
            compare(f'(c) from empty B {b} T {t} Hkv {hkv}', setting(False, off), on, 'fused forward on the projection', 'npm_mha_prefill_fwd (forced)')
            del cache, q, fresh
            D.trim_pool()
        print(f'last prefill kernel: {_C.last_prefill_kernel()}', flush=True)


if __name__ == '__main__':
    main()
