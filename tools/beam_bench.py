#!/usr/bin/env python3
"""What a beam step costs (npm_beam_step, beam.decode_step, PagedKVCache.reorder), in one process:

  1. npm_beam_step at G in {1, 8}, W in {4, 8}, V in {32000, 128256} on cold logits, against npm_sample_rows with top_k = 2 W
     (temperature 1, top_p 1) on the very same G W rows: that call runs the same passes -- maximum, the four-pass radix select
     for the 2 W-th key, the integer mass, a walk in index order -- without the ranking of the survivors and without the second
     launch that merges W lists.  Cold: the [G W, V] logit matrices of successive calls walk through one 512 MB region (twice
     the Infinity Cache).  Microseconds per call from HIP events around a window of back-to-back calls, launch gaps included;
     min / median / max over the windows, the two sides alternating.
  2. ``beam.decode_step`` against the plain one-token step (greedy ``Sampler``, embedding, ``decode``, head, the 4 bytes per
     sequence copied to the host) at B = G W, d 1024 / 8 heads / hidden 4096, V 32000, a paged cache of page 64 under a
     prompt of 512 rows: wall-clock microseconds per step, since both sides end in a host copy; and ``page_copies`` per step --
     the pages copy-on-write moved because beams share their tail page after a reorder.

    python tools/beam_bench.py > profiles/r20_beam_bench.log
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--g', default='1,8')
    ap.add_argument('--w', default='4,8')
    ap.add_argument('--v', default='32000,128256')
    ap.add_argument('--region-mb', type=int, default=512)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--calls', type=int, default=64, help='calls per window')
    ap.add_argument('--steps', type=int, default=48, help='decode steps per timed run')
    ap.add_argument('--prompt', type=int, default=512)
    a = ap.parse_args()

    import np_modeling_amd as npm
    from np_modeling_amd import _C, beam, device as D
    lib = _C.lib()
    groups, widths = [int(x) for x in a.g.split(',')], [int(x) for x in a.w.split(',')]
    print(f'beam_bench: sources {_C.source_id()}; {a.windows} windows of {a.calls} calls per kernel, alternating, after untimed ones; '
          f'logits walk a {a.region_mb} MB region; microseconds per call', flush=True)

    # ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
    region_floats = a.region_mb * (1 << 20) // 4
    chunk = 1 << 22
    region = D.empty([region_floats])
    rng = np.random.default_rng(0)
    noise = D.from_host((4 * rng.standard_normal(chunk)).astype(np.float32))
    for at in range(0, region_floats, chunk):
        _C.check(lib.npm_d2d(region.ptr + 4 * at, noise.ptr, 4 * min(chunk, region_floats - at)), 'npm_d2d')

    def window(fn, calls):
        start = D.Event().record()
        for _ in range(calls):
            fn()
        stop = D.Event().record()
        stop.synchronize()
        return start.elapsed_ms(stop) * 1e3 / calls

    fmt = lambda ts: f'{min(ts):8.1f} {sorted(ts)[len(ts) // 2]:8.1f} {max(ts):8.1f}'
    print(f'{"G":>2} {"W":>2} {"V":>7} | {"npm_beam_step min/med/max":>27} | {"npm_sample_rows k=2W min/med/max":>32} | {"beam/sample":>11} | kernel')
    for g in groups:
        for w in widths:
            for vocab in (int(x) for x in a.v.split(',')):
                n, c = g * w, 2 * w
                slots = region_floats // (n * vocab)
                params = D.bytes_from_host(np.concatenate([
                    np.arange(n, dtype=np.uint64).view(np.uint8), np.zeros(n, dtype=np.uint64).view(np.uint8),
                    np.full(n, 1.0, dtype=np.float32).view(np.uint8), np.full(n, c, dtype=np.int32).view(np.uint8),
                    np.full(n, 1.0, dtype=np.float32).view(np.uint8)]))
                q = params.ptr
                out = D.ByteBuffer(4 * (3 * n + 3 * g * c))
                cum_host = rng.uniform(-3, 0, size=n).astype(np.float32)
                cum = D.bytes_from_host(cum_host)
                work = D.ByteBuffer(_C.beam_workspace_bytes(g, w))
                state = {'at': 0}

                def logits():
                    state['at'] = (state['at'] + 1) % slots
                    return region.ptr + 4 * state['at'] * n * vocab

                def sample():
                    desc = _C.npm_sample(logits=logits(), pitch=vocab, batch=n, vocab=vocab, temperature=q + 16 * n, top_k=q + 20 * n,
                                         top_p=q + 24 * n, seed=q, draw=q + 8 * n, token=out.ptr, kept=out.ptr + 4 * n, prob=out.ptr + 8 * n)
                    _C.check(lib.npm_sample_rows(C.byref(desc)), 'npm_sample_rows')

                def beam_step():
                    # the running scores are written in place: every beam stays live, as in a search that has not finished
                    desc = _C.npm_beam(logits=logits(), pitch=vocab, groups=g, width=w, vocab=vocab, eos=2, cum=cum.ptr, parent=out.ptr,
                                       ids=out.ptr + 4 * n, lse=out.ptr + 8 * n, cand_slot=out.ptr + 12 * n,
                                       cand_token=out.ptr + 12 * n + 4 * g * c, cand_score=out.ptr + 12 * n + 8 * g * c,
                                       workspace=work.ptr, workspace_bytes=work.nbytes)
                    _C.check(lib.npm_beam_step(C.byref(desc)), 'npm_beam_step')

                times = {beam_step: [], sample: []}
                for fn in times:
                    window(fn, 8)
                for _ in range(a.windows):
                    for fn in times:
                        times[fn].append(window(fn, a.calls))
                    _C.check(lib.npm_h2d(cum.ptr, cum_host.ctypes.data, cum_host.nbytes), 'npm_h2d')     # scores only ever fall
                ratio = sorted(times[beam_step])[a.windows // 2] / sorted(times[sample])[a.windows // 2]
                print(f'{g:>2} {w:>2} {vocab:>7} | {fmt(times[beam_step]):>27} | {fmt(times[sample]):>32} | {ratio:>11.2f} | '
                      f'{_C.last_beam_kernel()}', flush=True)
    del region
    D.trim_pool()

    # ---- 2. the step -------------------------------------------------------------------------------------------------------------------
    f, hidden, vocab, page = 1024, 4096, 32000, 64
    print(f'\ndecode step, d {f} Hq 8 Hkv 8 hidden {hidden}, V {vocab}, paged cache of page {page}, prompt {a.prompt} rows, '
          f'{a.steps} steps per run; wall-clock microseconds per step, min / median / max over {a.windows} runs', flush=True)
    print(f'{"G":>2} {"W":>2} {"B":>3} | {"plain step min/med/max":>27} | {"beam.decode_step min/med/max":>29} | {"beam/plain":>10} | '
          f'{"page_copies/step":>16} {"pages in use":>12} {"of un-shared":>12}', flush=True)
    for g in groups:
        for w in widths:
            b = g * w
            np.random.seed(0)
            dec = npm.layers.TransformerDecoder(num_heads=8, hidden_units=hidden, norm_first=True, causal=True)
            rng = np.random.default_rng(1)
            kv = rng.standard_normal([b, 128, f]).astype(np.float32)
            dec(np.zeros([b, 2, f], dtype=np.float32), kv)
            emb = npm.layers.Embedding(vocab, f)
            emb(np.zeros([1], dtype=np.int64))
            head = npm.layers.Linear(units=vocab)
            head(np.zeros([1, f], dtype=np.float32))
            capacity = a.prompt + a.steps + 1
            prompt = rng.integers(0, vocab, size=[b, a.prompt])

            def plain_run():
                state = dec.start_decoding(kv, capacity, page_size=page)
                sampler = npm.sampling.Sampler(b)
                hidden_rows = dec.decode(emb.forward(prompt), state)
                logits = head(D.take_rows(hidden_rows.reshape(-1, f), np.arange(b) * a.prompt + a.prompt - 1))
                D.synchronize()
                start = time.perf_counter()
                for _ in range(a.steps):
                    result = sampler(logits)
                    x = emb.forward(result.ids).reshape(b, 1, f)
                    logits = head(dec.decode(x, state).reshape(b, f))
                    result.numpy()
                D.synchronize()
                return (time.perf_counter() - start) * 1e6 / a.steps, 0.0, state.self_cache.pages_in_use

            def beam_run():
                state = dec.start_decoding(kv, capacity, page_size=page)
                search = beam.BeamSearch(g, w)
                chunk_ids = np.full([b, a.prompt], -1, dtype=np.int64)
                chunk_ids[::w] = prompt[::w]
                n = np.zeros([b], dtype=np.int64)
                n[::w] = a.prompt
                beam.decode_step(dec, state, emb, head, search, prompt=(chunk_ids, n))
                D.synchronize()
                copies = state.self_cache.page_copies
                start = time.perf_counter()
                for _ in range(a.steps):
                    beam.decode_step(dec, state, emb, head, search)
                D.synchronize()
                took = (time.perf_counter() - start) * 1e6 / a.steps
                return took, (state.self_cache.page_copies - copies) / a.steps, state.self_cache.pages_in_use

            plain_run(), beam_run()                                          # untimed: code objects, first touch
            runs = {plain_run: [], beam_run: []}
            for _ in range(a.windows):
                for fn in runs:
                    runs[fn].append(fn())
            plain, beams = ([r[0] for r in runs[fn]] for fn in (plain_run, beam_run))
            ratio = sorted(beams)[a.windows // 2] / sorted(plain)[a.windows // 2]
            print(f'{g:>2} {w:>2} {b:>3} | {fmt(plain):>27} | {fmt(beams):>29} | {ratio:>10.2f} | {runs[beam_run][-1][1]:>16.2f} '
                  f'{runs[beam_run][-1][2]:>12d} {runs[plain_run][-1][2]:>12d}', flush=True)
            del dec, emb, head
            D.trim_pool()


if __name__ == '__main__':
    main()
