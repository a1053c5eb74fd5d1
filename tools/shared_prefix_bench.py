#!/usr/bin/env python3
"""The attention part of a decode step over B sequences forked from one prompt: one pass over the shared prefix
(npm_mha_prefix_fwd + the paged call over the rows behind it + npm_attn_combine, what ``device.SHARED_PREFIX`` runs) against the
ordinary paged call on THE SAME forked cache -- same pools, same block table, same process, in alternating rounds.

    B 1 / 8 / 64, P 512 / 2048 / 8192 shared rows, 1 / 64 / 256 private rows behind them, T 1 and 4, Hq 8, Hkv 8 and 1, D 128,
    page 64, f32 and f16 pools.

Method of tools/decode_paged_bench.py: microseconds per call from HIP events around a window of back-to-back calls, median (and
min .. max) over the rounds; a round times the yardstick window and then the shared window.  The three launches of the shared path
are also timed one at a time, each in windows of its own (their sum is more than the back-to-back figure: launches overlap the
tail of the kernel before).  "Cold" K / V: call i of a window reads slot i % slots of two arenas, every slot a forked cache of
its own (pages of its own for prefix and suffixes); the line of a shape prints the slots and their total size, and a total below
the 256 MB Infinity Cache is NOT cold, whatever the rotation -- which is every shape with a short prefix.  In the yardstick the B
sequences read the same prefix pages B times: those re-reads may hit the caches, which an un-forked cache (B copies of the
prompt) would not.  That case is not measured here.

Also printed per shape: the pages the forked cache holds against B prompts filled on their own.

    python tools/shared_prefix_bench.py > profiles/r19_shared_prefix_bench.log
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARENA_BYTES = 1 << 30
MAX_SLOTS = 24


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--b', default='1,8,64')
    ap.add_argument('--prefix', default='512,2048,8192')
    ap.add_argument('--suffix', default='1,64,256')
    ap.add_argument('--t', default='1,4')
    ap.add_argument('--kv', default='8,1')
    ap.add_argument('--dtype', default='f32,f16')
    ap.add_argument('--h', type=int, default=8)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--page', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window-ms', type=float, default=3.0)
    ap.add_argument('--parts', type=int, default=1, help='0: skip the one-at-a-time timings of the three launches')
    a = ap.parse_args()

    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    h, d, page = a.h, a.d, a.page
    scale = 1.0 / np.sqrt(d)
    ints = lambda s: [int(x) for x in s.split(',')]
    print(f'shared_prefix_bench: sources {_C.source_id()}, Hq {h} D {d} page {page}; {a.rounds} alternating rounds of ~{a.window_ms} ms '
          f'windows after untimed ones; microseconds per call, median (min .. max)', flush=True)
    print('columns: yardstick = the paged call on the forked cache | shared = suffix call + prefix pass + combine back to back | '
          'ratio shared / yardstick | the three launches alone: suffix, prefix (splits), combine | pages held forked / un-forked',
          flush=True)

    def window(fn, calls):
        start = D.Event().record()
        for i in range(calls):
            fn(i)
        stop = D.Event().record()
        stop.synchronize()
        return start.elapsed_ms(stop) * 1e3 / calls

    def calls_for(fn):
        window(fn, 8)
        us = window(fn, 8)
        return int(max(8, min(4000, a.window_ms * 1e3 / max(us, 1.0))))

    def med(t):
        t = sorted(t)
        return t[len(t) // 2], t[0], t[-1]

    ka, va = D.full([ARENA_BYTES // 4], 0.01), D.full([ARENA_BYTES // 4], 0.02)
    for dtype in a.dtype.split(','):
        size = 2 if dtype == 'f16' else 4
        for hkv in ints(a.kv):
            row = hkv * d
            page_bytes = page * row * size
            arena_pages = ARENA_BYTES // page_bytes
            for b in ints(a.b):
                for prefix in ints(a.prefix):
                    for suffix in ints(a.suffix):
                        for t in ints(a.t):
                            rows = suffix + t - 1                        # rows behind the prefix with the T new tokens included
                            shared, own = prefix // page, -(-rows // page)
                            slot_pages = shared + b * own
                            slots = int(max(1, min(MAX_SLOTS, arena_pages // slot_pages)))
                            per = shared + own
                            tables = np.empty([slots, b, per], dtype=np.int32)
                            for s in range(slots):
                                base = s * slot_pages
                                tables[s, :, :shared] = base + np.arange(shared)
                                tables[s, :, shared:] = base + shared + np.arange(b * own).reshape(b, own)
                            tab = D.bytes_from_host(tables)
                            lens = D.bytes_from_host(np.stack([np.full(b, prefix + rows), np.full(b, rows), np.full(b, t)]).astype(np.int32))
                            full_lens, behind, new = lens.ptr, lens.ptr + 4 * b, lens.ptr + 8 * b
                            q = D.from_host(np.random.default_rng(0).standard_normal([b, t, h, d]).astype(np.float32))
                            ctx, lse = D.empty([b, t, h, d]), D.empty([b, h, t])
                            splits = int(lib.npm_mha_prefix_splits(b * t, h, hkv, prefix))
                            part = D.empty([splits * b * t * h * (d + 1)])
                            part_lse = part.ptr + 4 * splits * b * t * h * d
                            dec = _C.npm_mha_decode()
                            dec.batch, dec.heads, dec.kv_heads, dec.new_tokens, dec.head_dim = b, h, hkv, t, d
                            dec.causal, dec.scale = 1, scale
                            dec.q, dec.q_pitch, dec.ctx, dec.ctx_pitch, dec.lse = q.ptr, h * d, ctx.ptr, h * d, lse.ptr
                            dec.k, dec.v = ka.ptr, va.ptr
                            dec.k_pitch = dec.v_pitch = row
                            dec.k_stride_b = dec.v_stride_b = page * row
                            assert h // hkv * t <= 32, 'the suffix call of this bench is the decode kernel'
                            f16 = int(dtype == 'f16')

                            def paged(table, lengths, kv_len):
                                dec.kv_len = kv_len
                                if f16:
                                    _C.check(lib.npm_mha_decode_fwd_f16(C.byref(dec), lengths, new, table, per, page), 'npm_mha_decode_fwd_f16')
                                else:
                                    _C.check(lib.npm_mha_decode_fwd_paged(C.byref(dec), lengths, new, table, per, page), 'npm_mha_decode_fwd_paged')

                            def table_of(i):
                                return tab.ptr + 4 * b * per * (i % slots)

                            def yardstick(i):
                                paged(table_of(i), full_lens, prefix + rows)

                            def suffix_call(i):
                                paged(table_of(i) + 4 * shared, behind, rows)

                            def prefix_call(i):
                                _C.check(lib.npm_mha_prefix_fwd(C.byref(dec), new, table_of(i), page, prefix, splits, part.ptr, part_lse, f16),
                                         'npm_mha_prefix_fwd')

                            def combine_call(i):
                                _C.check(lib.npm_attn_combine(part.ptr, part_lse, splits, ctx.ptr, h * d, lse.ptr, b, t, h, d, new, 0),
                                         'npm_attn_combine')

                            def shared_path(i):
                                suffix_call(i)
                                prefix_call(i)
                                combine_call(i)

                            n_off, n_on = calls_for(yardstick), calls_for(shared_path)
                            off, on = [], []
                            for _ in range(a.rounds):
                                off.append(window(yardstick, n_off))
                                on.append(window(shared_path, n_on))
                            off, on = med(off), med(on)
                            alone = ''
                            if a.parts:
                                each = [med([window(fn, calls_for(fn)) for _ in range(3)])[0] for fn in (suffix_call, prefix_call, combine_call)]
                                alone = f' | alone {each[0]:7.1f} {each[1]:7.1f} ({splits:3d}) {each[2]:6.1f}'
                            held, unforked = shared + b * own, b * -(-(prefix + rows) // page)
                            mb = slots * slot_pages * page_bytes * 2 / 2 ** 20
                            print(f'{dtype} Hkv {hkv} B {b:2d} P {prefix:4d} suffix {suffix:3d} T {t} | yardstick {off[0]:7.1f} ({off[1]:7.1f} .. {off[2]:7.1f}) '
                                  f'| shared {on[0]:7.1f} ({on[1]:7.1f} .. {on[2]:7.1f}) | ratio {on[0] / off[0]:5.2f}{alone} '
                                  f'| pages {held:5d} / {unforked:5d} | {slots:2d} slots {mb:6.0f} MB{"" if mb >= 256 else " (not cold)"}', flush=True)
                            del tab, lens, q, ctx, lse, part


if __name__ == '__main__':
    main()
