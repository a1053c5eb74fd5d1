#!/usr/bin/env python3
"""What a speculative step costs (sampling.NgramDrafter, Sampler.verify, speculative.decode_step), at d 1024 / 8 heads / hidden
4096, B in {1, 8}, T in {3, 7}, in one process:

  1. ``TransformerDecoder.decode`` of T + 1 rows per sequence against the one-row step, over a cache of L rows (after every call
     ``DecodeState.truncate`` takes the rows out again -- host state only -- so that every call sees the same L);
  2. npm_verify_rows on B (T + 1) logit rows against T + 1 calls of npm_sample_rows on B rows, at V 32000 and 128256
     (temperature 0.8, top-k 50, top-p 0.9: every pass of the row kernel runs);
  3. npm_ngram_draft over histories of 8192 tokens: ids drawn from a vocabulary of 32000 (hardly an n-gram repeats: every n from
     nmax down to nmin is searched) and from 4 tokens (the first n matches).

Times are microseconds per call from HIP events around a window of back-to-back calls, launch gaps included (what a user waits
for); min / median / max over the windows, the two sides of a comparison alternating.  Break-even: a speculative step emits
1 + a tokens where the plain step emits 1, so it pays once the mean number of accepted drafts a exceeds step(T + 1) / step(1) - 1;
the second figure adds the verify and draft launches to the speculative side and one npm_sample_rows to the plain side.  The
host copies and the vocabulary projection (B (T + 1) rows instead of B) are not in either figure.

    python tools/spec_bench.py > profiles/r18_spec_bench.log
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--b', default='1,8')
    ap.add_argument('--t', default='3,7')
    ap.add_argument('--vocab', default='32000,128256')
    ap.add_argument('--l', type=int, default=2048, help='cache rows under the decode step')
    ap.add_argument('--history', type=int, default=8192)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=20.0, help='calls per window are sized so that a window lasts about this long')
    a = ap.parse_args()

    import np_modeling_amd as npm
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    try:
        head = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True,
                              cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip() or 'unknown'
    except OSError:
        head = 'unknown'
    print(f'spec_bench: commit {head} (+ working tree), sources {_C.source_id()}; {a.windows} windows of ~{a.window_ms} ms after '
          'untimed ones; microseconds per call, min / median / max', flush=True)
    batches, drafts = [int(x) for x in a.b.split(',')], [int(x) for x in a.t.split(',')]

    def window(fn, calls):
        start = D.Event().record()
        for _ in range(calls):
            fn()
        stop = D.Event().record()
        stop.synchronize()
        return start.elapsed_ms(stop) * 1e3 / calls

    def measure(fns):
        """min / median / max per function, the functions' windows alternating."""
        calls = []
        for fn in fns:
            window(fn, 4)                                             # untimed: code objects, first touch
            us = window(fn, 4)
            calls.append(int(max(4, min(4000, a.window_ms * 1e3 / max(us, 1.0)))))
            window(fn, calls[-1])
        times = [[] for _ in fns]
        for _ in range(a.windows):
            for i, fn in enumerate(fns):
                times[i].append(window(fn, calls[i]))
        return [(min(t), sorted(t)[len(t) // 2], max(t)) for t in times]

    fmt = lambda t: f'{t[0]:8.1f} {t[1]:8.1f} {t[2]:8.1f}'

    # ---- 1. the decode step ------------------------------------------------------------------------------------------------------------
    f, hidden = 1024, 4096
    step = {}
    print(f'\ndecode step, d {f} Hq 8 Hkv 8 hidden {hidden}, L {a.l}', flush=True)
    print(f'{"B":>3} {"T":>2} | {"step(1) min/med/max":>26} | {"step(T + 1) min/med/max":>26} | {"ratio":>6} {"break-even a":>12}', flush=True)
    for b in batches:
        np.random.seed(0)
        layer = npm.layers.TransformerDecoder(num_heads=8, hidden_units=hidden, norm_first=True, causal=True)
        rng = np.random.default_rng(1)
        kv = rng.standard_normal([b, 128, f]).astype(np.float32)
        layer(np.zeros([b, 2, f], dtype=np.float32), kv)
        state = layer.start_decoding(kv, a.l + 64)
        layer.decode((0.1 * rng.standard_normal([b, a.l, f])).astype(np.float32), state)      # prefill
        for t in drafts:
            one = D.from_host((0.1 * rng.standard_normal([b, 1, f])).astype(np.float32))
            chunk = D.from_host((0.1 * rng.standard_normal([b, t + 1, f])).astype(np.float32))

            def run(x, rows):
                layer.decode(x, state)
                state.truncate(rows)

            t1, tn = measure([lambda: run(one, 1), lambda: run(chunk, t + 1)])
            step[b, t] = (t1[1], tn[1])
            print(f'{b:3d} {t:2d} | {fmt(t1)} | {fmt(tn)} | {tn[1] / t1[1]:6.3f} {tn[1] / t1[1] - 1:12.3f}', flush=True)
        del layer, state
        D.trim_pool()

    # ---- 2. verify against T + 1 sample calls ------------------------------------------------------------------------------------------
    verify = {}
    print('\nnpm_verify_rows on B (T + 1) rows against T + 1 npm_sample_rows on B rows; t 0.8, top-k 50, top-p 0.9', flush=True)
    print(f'{"V":>6} {"B":>3} {"T":>2} | {"one sample min/med/max":>26} | {"T + 1 samples min/med/max":>26} | {"verify min/med/max":>26} | '
          f'{"verify / samples":>16}', flush=True)
    for vocab in (int(x) for x in a.vocab.split(',')):
        for b in batches:
            for t in drafts:
                rows = t + 1
                rng = np.random.default_rng(vocab + b + t)
                logits = D.from_host((3 * rng.standard_normal([b * rows, vocab])).astype(np.float32))
                params = D.bytes_from_host(np.concatenate([
                    np.arange(1, b + 1, dtype=np.uint64).view(np.uint8), np.zeros([b], dtype=np.uint64).view(np.uint8),
                    np.full([b], 0.8, dtype=np.float32).view(np.uint8), np.full([b], 50, dtype=np.int32).view(np.uint8),
                    np.full([b], 0.9, dtype=np.float32).view(np.uint8)]))
                p = params.ptr
                common = dict(seed=p, draw=p + 8 * b, temperature=p + 16 * b, top_k=p + 20 * b, top_p=p + 24 * b)
                out = D.ByteBuffer(4 * (3 * b * rows + b))
                draft = D.ids_from_host(np.zeros([b, max(t, 1)], dtype=np.int32))
                n_draft = D.ids_from_host(np.full([b], t, dtype=np.int32))
                sample = [_C.npm_sample(logits=logits.ptr + 4 * r * vocab, pitch=rows * vocab, batch=b, vocab=vocab, active=None,
                                        token=out.ptr, kept=out.ptr + 4 * b, prob=out.ptr + 8 * b, **common) for r in range(rows)]
                desc = _C.npm_verify(logits=logits.ptr, pitch=vocab, batch=b, rows=rows, vocab=vocab, history_cap=0, draft=draft.ptr,
                                     draft_pitch=max(t, 1), n_draft=n_draft.ptr, token=out.ptr, accepted=out.ptr + 4 * b * rows,
                                     kept=out.ptr + 4 * (b * rows + b), prob=out.ptr + 4 * (2 * b * rows + b), history=None,
                                     history_pitch=0, history_len=None, **common)

                def run_one():
                    _C.check(lib.npm_sample_rows(C.byref(sample[0])), 'npm_sample_rows')

                def run_samples():
                    for s in sample:
                        _C.check(lib.npm_sample_rows(C.byref(s)), 'npm_sample_rows')

                def run_verify():
                    _C.check(lib.npm_verify_rows(C.byref(desc)), 'npm_verify_rows')

                t_one, t_all, t_ver = measure([run_one, run_samples, run_verify])
                verify[vocab, b, t] = (t_one[1], t_ver[1])
                print(f'{vocab:6d} {b:3d} {t:2d} | {fmt(t_one)} | {fmt(t_all)} | {fmt(t_ver)} | {t_ver[1] / t_all[1]:16.3f}', flush=True)
                del logits
            D.trim_pool()

    # ---- 3. the draft ------------------------------------------------------------------------------------------------------------------
    draft_us = {}
    print(f'\nnpm_ngram_draft, histories of {a.history} tokens, ngram (3, 1)', flush=True)
    print(f'{"B":>3} {"T":>2} {"ids":>8} | {"min/med/max":>26} | {"mean drafted":>12}', flush=True)
    for b in batches:
        for t in drafts:
            for name, alphabet in (('of 32000', 32000), ('of 4', 4)):
                rng = np.random.default_rng(b + t)
                history = D.ids_from_host(rng.integers(0, alphabet, size=[b, a.history]).astype(np.int32))
                lens = D.ids_from_host(np.full([b], a.history, dtype=np.int32))
                out = D.IdBuffer([b * (t + 1) + b])

                def run_draft():
                    _C.check(lib.npm_ngram_draft(history.ptr, a.history, a.history, lens.ptr, None, b, t, 3, 1, out.ptr,
                                                 out.ptr + 4 * b * (t + 1)), 'npm_ngram_draft')

                (t_draft,) = measure([run_draft])
                draft_us[b, t, name] = t_draft[1]
                drafted = out.numpy()[b * (t + 1):] - 1
                print(f'{b:3d} {t:2d} {name:>8} | {fmt(t_draft)} | {drafted.mean():12.2f}', flush=True)

    # ---- break-even --------------------------------------------------------------------------------------------------------------------
    print('\nbreak-even accepted drafts per step: decode alone, and with draft (ids of 32000) + verify against one sample', flush=True)
    for vocab in (int(x) for x in a.vocab.split(',')):
        for b in batches:
            for t in drafts:
                s1, sn = step[b, t]
                one, ver = verify[vocab, b, t]
                whole = (sn + ver + draft_us[b, t, 'of 32000']) / (s1 + one) - 1
                print(f'V {vocab:6d} B {b:2d} T {t}: decode alone {sn / s1 - 1:6.3f}, whole step {whole:6.3f} (of at most {t})', flush=True)


if __name__ == '__main__':
    main()
