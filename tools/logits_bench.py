#!/usr/bin/env python3
"""What the logit processors cost (npm_logits_process, npm_logprob_rows, speculative.decode_step(processor=)), in one process:

  1. npm_logits_process at B in {1, 8, 64}, V in {32000, 128256}, a history of 512 / 8192 random tokens per slot (half of it
     prompt), rows 1 and 8 (a speculative chunk whose draft is fully used), with and without a 256-entry bias list; repetition
     1.3, frequency 0.1, presence 0.7 -- against npm_sample_rows (temperature 0.8, top_k 50, top_p 0.9) on the very same
     B * rows cold rows, the launch it precedes.  Cold: the logit matrices of successive calls walk through one region of
     1 GB (four times the Infinity Cache); at B 64, rows 8, V 128256 one call covers 262 MB of it.  Microseconds per call from
     HIP events around a window of back-to-back calls, launch gaps included; min / median / max over the windows, the two sides
     alternating.  The processor edits in place, so later windows see logits that were processed before: the work does not
     depend on the values.
  2. npm_logprob_rows with top_n 0 / 5 / 20 against npm_beam_step at width 1 on the same cold rows: the same row kernel, the
     beam with its second (merge) launch.
  3. ``speculative.decode_step`` with and without a ``LogitProcessor`` at B 8, T 4, d 1024 / 8 heads / hidden 4096, V 32000, a
     paged cache of page 64 under a periodic prompt of 128 rows: wall-clock microseconds per step (a step ends in a host copy).

    python tools/logits_bench.py > profiles/r21_logits_bench.log
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
    ap.add_argument('--b', default='1,8,64')
    ap.add_argument('--v', default='32000,128256')
    ap.add_argument('--l', default='512,8192')
    ap.add_argument('--rows', default='1,8')
    ap.add_argument('--region-mb', type=int, default=1024)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--calls', type=int, default=24, help='calls per window')
    ap.add_argument('--steps', type=int, default=24, help='decode steps per timed run')
    a = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(',')]

    import np_modeling_amd as npm
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    print(f'logits_bench: sources {_C.source_id()}; {a.windows} windows of {a.calls} calls per kernel, alternating, after untimed ones; '
          f'logits walk a {a.region_mb} MB region; microseconds per call', flush=True)

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

    def measure(fns):
        times = {fn: [] for fn in fns}
        for fn in fns:
            window(fn, 4)
        for _ in range(a.windows):
            for fn in fns:
                times[fn].append(window(fn, a.calls))
        return [times[fn] for fn in fns]

    fmt = lambda ts: f'{min(ts):8.1f} {sorted(ts)[len(ts) // 2]:8.1f} {max(ts):8.1f}'
    med = lambda ts: sorted(ts)[len(ts) // 2]

    # ---- 1. the processor against the sampler it precedes ---------------------------------------------------------------------------------
    print(f'{"B":>2} {"rows":>4} {"V":>7} {"L":>5} {"bias":>4} | {"npm_logits_process min/med/max":>30} | {"npm_sample_rows min/med/max":>28} | '
          f'{"process/sample":>14}', flush=True)
    for b in ints(a.b):
        for rows in ints(a.rows):
            for vocab in ints(a.v):
                n = b * rows
                slots = max(1, region_floats // (n * vocab))
                state = {'at': 0}

                def logits():
                    state['at'] = (state['at'] + 1) % slots
                    return region.ptr + 4 * state['at'] * n * vocab

                sample_params = D.bytes_from_host(np.concatenate([
                    np.arange(n, dtype=np.uint64).view(np.uint8), np.zeros(n, dtype=np.uint64).view(np.uint8),
                    np.full(n, 0.8, dtype=np.float32).view(np.uint8), np.full(n, 50, dtype=np.int32).view(np.uint8),
                    np.full(n, 0.9, dtype=np.float32).view(np.uint8)]))
                q = sample_params.ptr
                out = D.ByteBuffer(12 * n)
                workspace = D.IdBuffer([b, vocab])
                _C.check(lib.npm_fill_f32(workspace.ptr, 0.0, b * vocab), 'npm_fill_f32')

                def sample():
                    desc = _C.npm_sample(logits=logits(), pitch=vocab, batch=n, vocab=vocab, temperature=q + 16 * n, top_k=q + 20 * n,
                                         top_p=q + 24 * n, seed=q, draw=q + 8 * n, token=out.ptr, kept=out.ptr + 4 * n, prob=out.ptr + 8 * n)
                    _C.check(lib.npm_sample_rows(C.byref(desc)), 'npm_sample_rows')

                for length in ints(a.l):
                    history = D.ids_from_host(rng.integers(0, vocab, size=[b, length]))
                    lengths = D.ids_from_host(np.full([b], length))
                    prompt = D.ids_from_host(np.full([b], length // 2))
                    draft = D.ids_from_host(rng.integers(0, vocab, size=[b, max(rows - 1, 1)]))
                    n_draft = D.ids_from_host(np.full([b], rows - 1))
                    floats = D.bytes_from_host(np.concatenate([np.full(b, 1.3), np.full(b, 0.7), np.full(b, 0.1)]).astype(np.float32))
                    eos = D.ids_from_host(np.concatenate([np.full(b, 2), np.full(b, length)]))         # min_new = L: the rule applies
                    for bias_cap in (0, 256):
                        index = D.ids_from_host(np.stack([rng.permutation(vocab)[:256] for _ in range(b)]))
                        value = D.bytes_from_host(rng.standard_normal([b, 256]).astype(np.float32))
                        count = D.ids_from_host(np.full([b], 256))

                        def process():
                            desc = _C.npm_logits(logits=logits(), pitch=vocab, batch=b, rows=rows, vocab=vocab, history_cap=length,
                                                 history=history.ptr, history_pitch=length, history_len=lengths.ptr, prompt_len=prompt.ptr,
                                                 draft=draft.ptr, draft_pitch=max(rows - 1, 1), n_draft=n_draft.ptr, active=None,
                                                 repetition=floats.ptr, presence=floats.ptr + 4 * b, frequency=floats.ptr + 8 * b,
                                                 eos=eos.ptr, min_new=eos.ptr + 4 * b, bias_index=index.ptr if bias_cap else None,
                                                 bias_value=value.ptr if bias_cap else None, bias_count=count.ptr if bias_cap else None,
                                                 bias_cap=bias_cap, workspace=workspace.ptr)
                            _C.check(lib.npm_logits_process(C.byref(desc)), 'npm_logits_process')

                        t_process, t_sample = measure([process, sample])
                        assert not workspace.numpy().any(), 'the workspace is not zero after the calls'
                        print(f'{b:>2} {rows:>4} {vocab:>7} {length:>5} {bias_cap:>4} | {fmt(t_process):>30} | {fmt(t_sample):>28} | '
                              f'{med(t_process) / med(t_sample):>14.3f}', flush=True)

    # ---- 2. log-probabilities against the beam's row kernel ---------------------------------------------------------------------------------
    print(f'\n{"R":>2} {"V":>7} {"top_n":>5} | {"npm_logprob_rows min/med/max":>28} | {"npm_beam_step W=1 min/med/max":>29} | {"logprob/beam":>12} | kernel',
          flush=True)
    for r in (8, 64):
        for vocab in ints(a.v):
            slots = max(1, region_floats // (r * vocab))
            state = {'at': 0}

            def logits():
                state['at'] = (state['at'] + 1) % slots
                return region.ptr + 4 * state['at'] * r * vocab

            ids = D.ids_from_host(rng.integers(0, vocab, size=[r]))
            cum_host = np.zeros([r], dtype=np.float32)
            cum = D.bytes_from_host(cum_host)
            out = D.ByteBuffer(4 * (2 * r + 2 * r * 64 + 9 * r))
            work = D.ByteBuffer(_C.beam_workspace_bytes(r, 1))

            def beam_step():
                base = out.ptr + 4 * (2 * r + 2 * r * 64)
                desc = _C.npm_beam(logits=logits(), pitch=vocab, groups=r, width=1, vocab=vocab, eos=-1, cum=cum.ptr, parent=base,
                                   ids=base + 4 * r, lse=base + 8 * r, cand_slot=base + 12 * r, cand_token=base + 20 * r,
                                   cand_score=base + 28 * r, workspace=work.ptr, workspace_bytes=work.nbytes)
                _C.check(lib.npm_beam_step(C.byref(desc)), 'npm_beam_step')     # cum runs on: a few hundred finite steps

            for top_n in (0, 5, 20):
                def logprob():
                    desc = _C.npm_logprob(logits=logits(), pitch=vocab, rows=r, vocab=vocab, top_n=top_n, ids=ids.ptr, lse=out.ptr,
                                          chosen=out.ptr + 4 * r, top_token=out.ptr + 8 * r, top_logprob=out.ptr + 4 * (2 * r + r * 64))
                    _C.check(lib.npm_logprob_rows(C.byref(desc)), 'npm_logprob_rows')

                t_logprob, t_beam = measure([logprob, beam_step])
                logprob()
                print(f'{r:>2} {vocab:>7} {top_n:>5} | {fmt(t_logprob):>28} | {fmt(t_beam):>29} | {med(t_logprob) / med(t_beam):>12.2f} | '
                      f'{_C.last_beam_kernel()}', flush=True)
    del region
    D.trim_pool()

    # ---- 3. the speculative step ---------------------------------------------------------------------------------------------------------
    f, hidden, vocab, page, b, t, prompt_rows = 1024, 4096, 32000, 64, 8, 4, 128
    print(f'\nspeculative.decode_step, B {b}, T {t}, d {f} Hq 8 Hkv 8 hidden {hidden}, V {vocab}, paged cache of page {page}, periodic prompt of '
          f'{prompt_rows} rows, {a.steps} steps per run; wall-clock microseconds per step, min / median / max over {a.windows} runs', flush=True)
    np.random.seed(0)
    dec = npm.layers.TransformerDecoder(num_heads=8, hidden_units=hidden, norm_first=True, causal=True)
    kv = rng.standard_normal([b, 128, f]).astype(np.float32)
    dec(np.zeros([b, 2, f], dtype=np.float32), kv)
    emb = npm.layers.Embedding(vocab, f)
    emb(np.zeros([1], dtype=np.int64))
    head = npm.layers.Linear(units=vocab)
    head(np.zeros([1, f], dtype=np.float32))
    capacity = prompt_rows + (a.steps + 2) * (t + 1)
    prompts = [[int(v) for v in np.resize(rng.integers(0, vocab, size=7), prompt_rows)] for _ in range(b)]

    def run(with_processor):
        state = dec.start_decoding(kv, capacity, page_size=page)
        sampler = npm.sampling.Sampler(b)
        drafter = npm.sampling.NgramDrafter(b, capacity, t)
        proc = None
        if with_processor:
            proc = npm.sampling.LogitProcessor(b, vocab, max_bias=8)
            for s in range(b):
                proc.set(s, repetition_penalty=1.1, frequency_penalty=0.05, presence_penalty=0.1, logit_bias={5: -np.inf, 6: 0.5}, eos=2,
                         min_new_tokens=1000, prompt_length=prompt_rows)
        hidden_rows = dec.decode(emb.forward(np.array(prompts)), state)
        logits = head(D.take_rows(hidden_rows.reshape(-1, f), np.arange(b) * prompt_rows + prompt_rows - 1))
        for s in range(b):
            drafter.admit(s, prompts[s])
        drafter.append(sampler(logits if proc is None else proc(logits, drafter)))
        D.synchronize()
        start = time.perf_counter()
        emitted = 0
        for _ in range(a.steps):
            emitted += sum(len(o) for o in npm.speculative.decode_step(dec, state, emb, head, sampler, drafter, processor=proc))
        D.synchronize()
        return (time.perf_counter() - start) * 1e6 / a.steps, emitted / (a.steps * b)

    run(False), run(True)                                                    # untimed: code objects, first touch
    results = {False: [], True: []}
    for _ in range(a.windows):
        for flag in (False, True):
            results[flag].append(run(flag))
    plain, processed = ([r[0] for r in results[flag]] for flag in (False, True))
    print(f'without a processor {fmt(plain)} ({results[False][-1][1]:.2f} tokens per slot-step) | with one {fmt(processed)} '
          f'({results[True][-1][1]:.2f} tokens per slot-step) | with/without {med(processed) / med(plain):.3f}', flush=True)


if __name__ == '__main__':
    main()
