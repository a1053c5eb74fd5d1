#!/usr/bin/env python3
"""What the decode step of a decoder-only language model costs, and what the two things added for it buy, in one process:

  (a) npm_rope_kv_append against npm_rope + two npm_kv_append_paged on the SAME buffers (a packed projection of 8 + 2 x 8 heads of
      128, d 1024; a paged fp32 cache of 64-row pages), at B 1 / 8 / 64 with T 1 and at B 8 with T 512.  Microseconds per call from HIP
      events around a window of back-to-back calls; the variants alternate; median (min .. max) over the windows.
  (b) The ``models.CausalLM.decode`` step (one token per sequence, B 8, d 1024, 8 heads, hidden 2688, rms + swiglu + rope, page 64, 512
      rows cached) at 4 and 16 layers, three ways: the fused launch on (what the model does), the fused launch off (npm_rope and two
      appends per layer), and N single-layer states driven by hand -- ``TransformerDecoder(cross_attention=False).decode`` over N
      ``DecodeState`` s of its own, the loop a user had to write, with the three launches.  Wall-clock microseconds per step
      (the host's uploads are part of what is compared), a device synchronisation closing every window; the cache is truncated by
      one row after every step so that every step sees the same lengths.  The npm_h2d calls per step are counted by wrapping the
      library's entry point.

The yardsticks are the existing launches and the hand-driven loop, never the new code.  "spread": (max - min) / median over the
yardstick's own windows -- a difference below it is not a difference.  If the fused kernel is slower than the three launches beyond
that spread at a T 1 shape, say so where the figures are quoted and route that shape to the three launches.

    python tools/lm_decode_bench.py > profiles/lm_decode_bench.log
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEADS, KV_HEADS, HEAD_DIM, PAGE = 8, 8, 128, 64
FEATURES, HIDDEN, VOCAB = 1024, 2688, 32000


def _stats(values):
    v = np.sort(np.asarray(values, dtype=np.float64))
    return float(np.median(v)), float(v[0]), float(v[-1])


def _line(name, values, unit='us'):
    med, lo, hi = _stats(values)
    print(f'  {name:<44s} {med:10.2f} {unit} ({lo:.2f} .. {hi:.2f})  spread {(hi - lo) / max(med, 1e-9):.3f}', flush=True)
    return max(med, 1e-9)


def kernels(a, npm) -> None:
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    rng = np.random.default_rng(0)
    width, row = (HEADS + 2 * KV_HEADS) * HEAD_DIM, KV_HEADS * HEAD_DIM
    for batch, tokens in ((1, 1), (8, 1), (64, 1), (8, 512)):
        capacity = 1024
        pages_per = capacity // PAGE
        x = D.from_host(rng.standard_normal([batch * tokens, width]).astype(np.float32))
        pools = [D.empty([batch * pages_per, PAGE, KV_HEADS, HEAD_DIM]) for _ in range(2)]
        table = D.bytes_from_host(rng.permutation(batch * pages_per).reshape(batch, pages_per).astype(np.int32))
        lens = D.bytes_from_host(np.stack([np.full(batch, 300), np.full(batch, tokens)]).astype(np.int32))
        rope = D.RopeTable(HEAD_DIM, 10000.0).ensure(capacity)
        at_lens, new_lens = lens.ptr, lens.ptr + 4 * batch

        def three():
            _C.check(lib.npm_rope(x.ptr, width, batch, tokens, HEADS + KV_HEADS, HEAD_DIM, rope.cos.ptr, rope.sin.ptr, rope.rows, 0, at_lens, 0), 'npm_rope')
            for part, pool in ((HEADS * HEAD_DIM, pools[0]), (HEADS * HEAD_DIM + row, pools[1])):
                _C.check(lib.npm_kv_append_paged(x.ptr + 4 * part, width, pool.ptr, row, PAGE * row, batch, tokens, row, at_lens, new_lens,
                                                 table.ptr, pages_per, PAGE), 'npm_kv_append_paged')

        def fused():
            _C.check(lib.npm_rope_kv_append(x.ptr, width, batch, tokens, HEADS, KV_HEADS, HEAD_DIM, rope.cos.ptr, rope.sin.ptr, rope.rows, 0,
                                            at_lens, new_lens, pools[0].ptr, pools[1].ptr, row, PAGE * row, table.ptr, pages_per, PAGE, 0),
                     'npm_rope_kv_append')

        def window(fn):
            start = D.Event().record()
            for _ in range(a.calls):
                fn()
            stop = D.Event().record()
            stop.synchronize()
            return 1e3 * start.elapsed_ms(stop) / a.calls

        for fn in (three, fused):
            window(fn)
        times = {'three': [], 'fused': []}
        for _ in range(a.windows):
            times['three'].append(window(three))
            times['fused'].append(window(fused))
        print(f'(a) B {batch} T {tokens}: {lib.npm_last_rope_append_kernel().decode()}')
        base = _line('npm_rope + 2 npm_kv_append_paged (yardstick)', times['three'])
        got = _line('npm_rope_kv_append', times['fused'])
        print(f'  fused / three launches = {got / base:.3f}', flush=True)


def steps(a, npm) -> None:
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    batch, cached = 8, 512
    uploads = [0, 0]
    h2d = lib.npm_h2d

    def counting(dst, src, nbytes):
        uploads[0] += 1
        uploads[1] += int(nbytes)
        return h2d(dst, src, nbytes)

    for layers in (4, 16):
        np.random.seed(layers)
        lm = npm.models.CausalLM(VOCAB, FEATURES, layers, HEADS, HIDDEN)
        lm(np.zeros([batch, 2], dtype=np.int64))
        for block in lm.layers:
            for owner in (block._self_attention, block._dense1._linear, block._dense2):
                for name in ('_wq', '_wk', '_wv', '_wo', '_w'):
                    if hasattr(owner, name):
                        getattr(owner, name).set(np.asarray(getattr(owner, name)) / np.float32(np.sqrt(FEATURES)))
        rng = np.random.default_rng(1)
        prompt = rng.integers(0, VOCAB, [batch, cached])
        token = D.as_ids(rng.integers(0, VOCAB, [batch, 1]))

        def model_state():
            state = lm.start_decoding(batch, cached + 64, page_size=PAGE)
            lm.decode(prompt, state)
            return state

        def model_step(state):
            lm.decode(token, state)
            state.truncate(1)

        def hand_states():
            states = [block.start_decoding(None, cached + 64, batch=batch, page_size=PAGE) for block in lm.layers]
            x = lm.embedding.forward(prompt)
            for block, state in zip(lm.layers, states):
                x = block.decode(x, state)
            return states

        def hand_step(states):
            x = lm.embedding.forward(token)
            for block, state in zip(lm.layers, states):
                x = block.decode(x, state)
                state.truncate(1)
            hidden = lm.final_norm._forward_impl(x.reshape(batch, FEATURES))
            lm.head.forward(hidden)

        def window(fn, state):
            D.synchronize()
            start = time.perf_counter()
            for _ in range(a.steps):
                fn(state)
            D.synchronize()
            return 1e6 * (time.perf_counter() - start) / a.steps

        variants = {}
        lm.fused_rope_append = True
        variants['layered cache, fused launch'] = (model_step, model_state(), True)
        variants['layered cache, three launches'] = (model_step, model_state(), False)
        variants['N states by hand, three launches (yardstick)'] = (hand_step, hand_states(), False)
        times = {name: [] for name in variants}
        counts = {}
        for name, (fn, state, on) in variants.items():
            lm.fused_rope_append = on
            window(fn, state)
            uploads[:] = [0, 0]
            lib.npm_h2d = counting
            try:
                fn(state)
            finally:
                lib.npm_h2d = h2d
            counts[name] = tuple(uploads)
        for _ in range(a.windows):
            for name, (fn, state, on) in variants.items():
                lm.fused_rope_append = on
                times[name].append(window(fn, state))
        print(f'(b) {layers} layers, B {batch}, one token over {cached} cached rows, page {PAGE}:')
        medians = {name: _line(f'{name} [{counts[name][0]} npm_h2d, {counts[name][1]} B]', times[name]) for name in variants}
        base = medians['N states by hand, three launches (yardstick)']
        for name in list(variants)[:2]:
            print(f'  {name} / yardstick = {medians[name] / base:.3f}', flush=True)
        del variants


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--calls', type=int, default=200, help='(a) calls per timed window')
    ap.add_argument('--steps', type=int, default=20, help='(b) decode steps per timed window')
    ap.add_argument('--skip-steps', action='store_true')
    a = ap.parse_args()
    import np_modeling_amd as npm
    from np_modeling_amd import _C
    print(f'lm_decode_bench: sources {_C.source_id()}; {a.windows} windows per variant, alternating, after untimed calls; '
          f'median (min .. max)', flush=True)
    kernels(a, npm)
    if not a.skip_steps:
        steps(a, npm)


if __name__ == '__main__':
    main()
