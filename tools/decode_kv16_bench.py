#!/usr/bin/env python3
"""What storing K / V as fp16 buys the decode attention (npm_mha_decode_fwd_f16 against npm_mha_decode_fwd, csrc/npm_decode.hip) at
T = 1 new token, Hq 8, D 128, with the method of tools/decode_bench.py / tools/decode_paged_bench.py: time per call from HIP events
around a window of back-to-back calls (the combine launch included), min / median / max over the windows; "cold" K / V (every
call of a window reads a different slice of two arenas far larger than the 256 MB Infinity Cache; a K / V pair larger than that is
its own arena).  Same process, interleaved, per shape:

  (a) the fp32 entry point on an fp32 cache       the baseline (code and entry points unchanged), measured before and after (b)
  (b) the _f16 entry point on an fp16 cache       holding the same values (a constant that fp16 represents exactly)

on the grid of profiles/r08_decode_bench.log -- B 1 / 8 / 64, L 512 / 2048 / 8192, Hkv 8 / 2 / 1 -- then one paged row (page 64) and
one ragged draw (lengths uniform in 1 .. Lmax, seeded) at B 64, Lmax 8192, then one TransformerDecoder.decode step at B 1 and B 64
with either cache type.  Per row: microseconds, the ratio of the medians, the fraction of 8 TB/s on the K / V bytes actually read,
whether the fp16 median lies below (a)'s own minimum over both of its measurements, and the r08 median of the fp32 row.

    python tools/decode_kv16_bench.py > profiles/r14_decode_kv16_bench.log
    rocprofv3 --kernel-trace --stats -d DIR -o kv16 -- python tools/decode_kv16_bench.py --b 64 --l 2048 --kv 8 --no-step
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARENA_BYTES = 1 << 30
DENOM_TBS = 8.0
# profiles/r08_decode_bench.log, "decode cold" medians: (B, L, Hkv) -> microseconds
R08 = {(1, 512, 8): 15.6, (1, 512, 2): 15.1, (1, 512, 1): 14.5, (1, 2048, 8): 19.8, (1, 2048, 2): 18.7, (1, 2048, 1): 18.7,
       (1, 8192, 8): 40.5, (1, 8192, 2): 35.5, (1, 8192, 1): 31.1, (8, 512, 8): 17.0, (8, 512, 2): 15.8, (8, 512, 1): 15.4,
       (8, 2048, 8): 37.2, (8, 2048, 2): 20.1, (8, 2048, 1): 19.1, (8, 8192, 8): 98.4, (8, 8192, 2): 52.0, (8, 8192, 1): 38.1,
       (64, 512, 8): 49.4, (64, 512, 2): 19.1, (64, 512, 1): 16.5, (64, 2048, 8): 169.3, (64, 2048, 2): 54.8, (64, 2048, 1): 35.6,
       (64, 8192, 8): 662.6, (64, 8192, 2): 175.9, (64, 8192, 1): 95.2}
VALUE = 0.0099945068359375        # fp16 0x211e: the arenas of both types hold this value exactly


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--b', default='1,8,64')
    ap.add_argument('--l', default='512,2048,8192')
    ap.add_argument('--kv', default='8,2,1')
    ap.add_argument('--h', type=int, default=8)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=8.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--no-layouts', action='store_true', help='skip the paged and the ragged row')
    ap.add_argument('--no-step', action='store_true', help='skip the TransformerDecoder.decode step')
    a = ap.parse_args()

    import np_modeling_amd as npm
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    h, d = a.h, a.d
    scale = 1.0 / np.sqrt(d)
    half_bits = int(np.float16(VALUE).view(np.uint16))
    assert float(np.float16(VALUE)) == VALUE
    pair = float(np.array([half_bits | half_bits << 16], dtype=np.uint32).view(np.float32)[0])     # two such halves as one float
    print(f'decode_kv16_bench: sources {_C.source_id()}, Hq {h} D {d} T 1; {a.windows} windows of ~{a.window_ms} ms after one untimed '
          f'window; microseconds per call; K / V arenas of {ARENA_BYTES >> 20} MB each per type', flush=True)

    def window(fn, calls):
        start = D.Event().record()
        for i in range(calls):
            fn(i)
        stop = D.Event().record()
        stop.synchronize()
        return start.elapsed_ms(stop) * 1e3 / calls

    def measure(fn):
        calls = 8
        window(fn, calls)                                         # untimed: code objects, first touch
        us = window(fn, calls)
        calls = int(max(8, min(4000, a.window_ms * 1e3 / max(us, 1.0))))
        window(fn, calls)
        t = sorted(window(fn, calls) for _ in range(a.windows))
        return t[0], t[len(t) // 2], t[-1]

    class Shape:
        """The arenas, the descriptor and the calls of one (B, Lmax, Hkv) in both storage types."""

        def __init__(self, b, lmax, hkv):
            self.b, self.lmax, self.hkv = b, lmax, hkv
            self.elements = b * lmax * hkv * d                    # one of K, V
            self.arena = {}
            for dtype, size in (('f32', 4), ('f16', 2)):
                nbytes = max(ARENA_BYTES, self.elements * size)
                fill = VALUE if dtype == 'f32' else pair
                self.arena[dtype] = (D.full([nbytes // 4], fill), D.full([nbytes // 4], fill), max(1, nbytes // (self.elements * size)), size)
            q = D.from_host(np.random.default_rng(0).standard_normal([b, 1, h, d]).astype(np.float32))
            self.keep = (q, D.empty([b, 1, h, d]), D.empty([b, h, 1]))
            dec = self.dec = _C.npm_mha_decode()
            dec.batch, dec.heads, dec.kv_heads, dec.new_tokens, dec.kv_len, dec.head_dim = b, h, hkv, 1, lmax, d
            dec.causal, dec.scale = 1, scale
            dec.q, dec.q_pitch, dec.ctx, dec.ctx_pitch, dec.lse = q.ptr, h * d, self.keep[1].ptr, h * d, self.keep[2].ptr
            dec.k_pitch = dec.v_pitch = hkv * d

        def call(self, dtype, lengths=None, page_rows=0):
            """fn(i) of one layout: uniform (lengths None), ragged, or paged with the pages of a slice in a seeded random order."""
            ka, va, slots, size = self.arena[dtype]
            dec, b, lmax, hkv = self.dec, self.b, self.lmax, self.hkv
            lens = None if lengths is None else D.bytes_from_host(np.ascontiguousarray(np.asarray(lengths, dtype=np.int32)))
            tab, per = None, 0
            if page_rows:
                per = lmax // page_rows
                tab = D.bytes_from_host(np.random.default_rng(a.seed + page_rows).permutation(b * per).astype(np.int32))
            stride = (page_rows if page_rows else lmax) * hkv * d

            def run(i, lens=lens, tab=tab):
                off = size * self.elements * (i % slots)
                dec.k, dec.v, dec.k_stride_b, dec.v_stride_b = ka.ptr + off, va.ptr + off, stride, stride
                lp, tp = None if lens is None else lens.ptr, None if tab is None else tab.ptr
                if dtype == 'f16':
                    _C.check(lib.npm_mha_decode_fwd_f16(C.byref(dec), lp, None, tp, per, page_rows), 'npm_mha_decode_fwd_f16')
                elif tab is not None:
                    _C.check(lib.npm_mha_decode_fwd_paged(C.byref(dec), lp, None, tp, per, page_rows), 'npm_mha_decode_fwd_paged')
                elif lens is not None:
                    _C.check(lib.npm_mha_decode_fwd_varlen(C.byref(dec), lp, None), 'npm_mha_decode_fwd_varlen')
                else:
                    _C.check(lib.npm_mha_decode_fwd(C.byref(dec)), 'npm_mha_decode_fwd')
            return run

    slower = []

    def compare(shape, tag, keys, lengths=None, page_rows=0, r08=None):
        """(a), (b), (a) again for one layout; ``keys``: the K / V rows actually read."""
        t32 = measure(shape.call('f32', lengths, page_rows))
        t16 = measure(shape.call('f16', lengths, page_rows))
        t32b = measure(shape.call('f32', lengths, page_rows))
        lo, med = min(t32[0], t32b[0]), 0.5 * (t32[1] + t32b[1])
        read = 2.0 * keys * shape.hkv * d                         # elements of K and V
        where = 'below' if t16[1] < lo else 'NOT below'
        if t16[1] > max(t32[2], t32b[2]):
            slower.append(tag)
        print(f'{tag:<34} | f32 {t32[0]:7.1f} {t32[1]:7.1f} {t32[2]:7.1f}  again {t32b[0]:7.1f} {t32b[1]:7.1f} {t32b[2]:7.1f}  '
              f'{4 * read / med / 1e6 / DENOM_TBS:5.3f} of 8 TB/s{"" if r08 is None else f"  r08 {r08:6.1f}"} | f16 {t16[0]:7.1f} {t16[1]:7.1f} '
              f'{t16[2]:7.1f}  {2 * read / t16[1] / 1e6 / DENOM_TBS:5.3f} of 8 TB/s | f16 / f32 {t16[1] / med:5.3f}  median {where} the f32 '
              f'minimum {lo:.1f} | K + V MB {4 * read / 2 ** 20:7.1f} -> {2 * read / 2 ** 20:7.1f}', flush=True)

    print('columns: min med max per measurement; the fraction of 8 TB/s counts the K / V bytes of the valid rows in that storage type', flush=True)
    for b in (int(x) for x in a.b.split(',')):
        for length in (int(x) for x in a.l.split(',')):
            for hkv in (int(x) for x in a.kv.split(',')):
                shape = Shape(b, length, hkv)
                splits = lib.npm_mha_decode_splits(b, hkv, length)
                compare(shape, f'B {b:2d} L {length:4d} Hkv {hkv} splits {splits:2d}', b * length, r08=R08.get((b, length, hkv)) if (h, d) == (8, 128) else None)
                del shape
                D.trim_pool()
    if not a.no_layouts:
        b, lmax, hkv = 64, 8192, 8
        shape = Shape(b, lmax, hkv)
        full = np.full(b, lmax)
        compare(shape, f'B {b} Lmax {lmax} Hkv {hkv} paged 64', b * lmax, full, 64)
        draw = np.random.default_rng(a.seed).integers(1, lmax + 1, b)
        compare(shape, f'B {b} Lmax {lmax} Hkv {hkv} ragged', int(draw.sum()), draw)
        compare(shape, f'B {b} Lmax {lmax} Hkv {hkv} ragged paged 64', int(draw.sum()), draw, 64)
        del shape
        D.trim_pool()
    print('fp16 slower than fp32 beyond the spread at:', slower or 'no row', flush=True)

    if a.no_step:
        return
    # one decode step of a decoder layer with either cache type
    f, hidden, length = 1024, 4096, 2048
    for b in (1, 64):
        for dtype in ('f32', 'f16', 'f32'):
            np.random.seed(0)
            layer = npm.layers.TransformerDecoder(num_heads=8, hidden_units=hidden, norm_first=True, num_kv_heads=8, causal=True)
            rng = np.random.default_rng(1)
            kv = rng.standard_normal([b, 128, f]).astype(np.float32)
            layer(np.zeros([b, 2, f], dtype=np.float32), kv)
            state = layer.start_decoding(kv, length + 64, cache_dtype=dtype)
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
            print(f'decode step d {f} Hq 8 Hkv 8 B {b} L {state.position} cache {dtype}: {step_us:.1f} us per step (host clock of the stream); '
                  f'attention (mha_decode + kv_append) {att / total:.1%} of the kernel time; self cache {state.self_cache.nbytes / 2 ** 20:.1f} MB, '
                  f'cross cache {state.cross_cache.nbytes / 2 ** 20:.1f} MB; us per step: {parts}', flush=True)
            del layer, state
            D.trim_pool()


if __name__ == '__main__':
    main()
