#!/usr/bin/env python3
"""Times grouped-query attention's fused core (npm_mha_core_fwd_grouped / npm_mha_core_bwd_grouped) at the C5 attention shape
(B 256, S 512, Hq 8, D 128 by default) for several K / V head counts, next to the MHA call (npm_mha_core_fwd / _bwd) in the
same process.  Operands packed as the layer's self-attention keeps them ([B, S, Hq + 2 Hkv, D]); scores saved from head size 64
up, as the layer does.  FLOPs are counted on Hq (forward 2 products, backward 4); fp32-MFMA peak 157.3 TF as the denominator.

The group reduction (mha_gqa_reduce_kernel) runs inside npm_mha_core_bwd_grouped; its own time comes from a kernel trace:

    rocprofv3 --kernel-trace -d DIR -o gqa -- python tools/gqa_bench.py --kv 2 --reps 3
    python tools/gqa_bench.py --stats DIR/gqa_results.db      # the reduce kernel against the backward kernels
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TF = 157.3


def stats(path: str) -> None:
    """Per-kernel mean durations from a rocprofv3 kernel trace database (its `kernels` view): the reduce kernel against the
    rest of a grouped backward (row terms + the backward kernel)."""
    import sqlite3
    db = sqlite3.connect(path)
    pick = {}
    for name, calls, mean_ns in db.execute('SELECT name, COUNT(*), AVG(duration) FROM kernels GROUP BY name'):
        short = name.replace('void ', '').replace('(anonymous namespace)::', '').split('(')[0]
        if short.startswith(('mha_', )):
            pick[short] = (calls, mean_ns / 1e6)
    for name, (calls, ms) in sorted(pick.items()):
        print(f'{name:34s} {calls:4d} calls  mean {ms:.3f} ms')
    red = [ms for n, (_, ms) in pick.items() if n.startswith('mha_gqa_reduce_kernel')]
    bwd = [ms for n, (_, ms) in pick.items() if n.startswith('mha_bwd')]
    rows = [ms for n, (_, ms) in pick.items() if n.startswith(('mha_rowterms_kernel', 'mha_lse2_kernel'))]
    if red and bwd:
        whole = red[0] + bwd[0] + sum(rows)
        print(f'reduce {red[0]:.3f} ms = {red[0] / whole:.1%} of a grouped backward of {whole:.3f} ms in kernels '
              f'(backward kernel {bwd[0]:.3f}, row terms {sum(rows):.3f})')


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--b', type=int, default=256)
    ap.add_argument('--s', type=int, default=512)
    ap.add_argument('--h', type=int, default=8)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--kv', default='8,4,2,1', help='K / V head counts to time (the MHA call is timed first in any case)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warm', type=int, default=2)
    ap.add_argument('--stats', default='', help='summarise a rocprofv3 kernel trace database instead of timing')
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
        return

    import np_modeling_amd  # noqa: F401
    from np_modeling_amd import device as D
    from np_modeling_amd.device import Mat

    b, s, h, d = a.b, a.s, a.h, a.d
    save = D.attn_save_scores(d)
    scale = 1.0 / np.sqrt(d)
    rng = np.random.default_rng(0)
    print(f'B {b} S {s} Hq {h} D {d}, scores {"saved" if save else "recomputed"}, median of {a.reps} after {a.warm} untimed', flush=True)

    def run(hkv, grouped):
        width = (h + 2 * hkv) * d
        qkv = D.from_host(rng.standard_normal([b, s, h + 2 * hkv, d], dtype=np.float32))
        q, k, v = qkv, qkv.flat_view(h * d, [qkv.size - h * d]), qkv.flat_view((h + hkv) * d, [qkv.size - (h + hkv) * d])
        dctx = D.from_host(rng.standard_normal([b, s, h, d], dtype=np.float32))
        dqkv = D.empty([b, s, h + 2 * hkv, d])
        dq, dk, dv = dqkv, dqkv.flat_view(h * d, [dqkv.size - h * d]), dqkv.flat_view((h + hkv) * d, [dqkv.size - (h + hkv) * d])
        dims = (b, h, s, s, d)
        kv = hkv if grouped else None
        state = {}
        out = {}
        for name in ('fwd', 'bwd'):
            times, flops = [], 0.0
            for rep in range(a.warm + a.reps):
                with D.KernelTimer() as t:
                    if name == 'fwd':
                        state['fwd'] = D.mha_core_fwd(Mat(q, width), Mat(k, width), Mat(v, width), dims, scale, save_scores=save, kv_heads=kv)
                    else:
                        ctx, lse, scores = state['fwd']
                        D.mha_core_bwd(Mat(q, width), Mat(k, width), Mat(v, width), ctx, lse, dctx, Mat(dq, width), Mat(dk, width),
                                       Mat(dv, width), dims, scale, scores=scores, kv_heads=kv)
                rec = list(t.summary().values())[0]
                if rep >= a.warm:
                    times.append(rec['ms'])
                    flops = rec['flops']
            ms = float(np.median(times))
            out[name] = ms
            tf = flops / ms / 1e9
            label = 'MHA' if not grouped else f'Hkv {hkv}'
            print(f'{label:7s} {name}: {ms:.3f} ms (min {min(times):.3f})  {tf:.1f} TF  ({tf / PEAK_TF:.1%} of peak)', flush=True)
        del qkv, dqkv, dctx, state
        return out

    base = run(h, grouped=False)
    for hkv in (int(x) for x in a.kv.split(',')):
        got = run(hkv, grouped=True)
        print(f'Hkv {hkv}: fwd {got["fwd"] / base["fwd"] - 1:+.1%}, bwd {got["bwd"] / base["bwd"] - 1:+.1%} against MHA', flush=True)


if __name__ == '__main__':
    main()
