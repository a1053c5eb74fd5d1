#!/usr/bin/env python3
"""What the RMSNorm and gated-SiLU ("SwiGLU") kernels cost, in one process:

  1. npm_rmsnorm_fwd / _bwd against npm_layernorm_fwd / _bwd on the SAME buffers at [131072, 1024] and [65536, 4096] (the backward with
     a residual, as the pre-norm block calls it).  The LayerNorm kernels are the yardstick: unchanged code that moves the same bytes.
     "spread": (max - min) / median over the yardstick's own windows -- a difference below it is not a difference.
  2. npm_swiglu_fwd / _bwd at [131072, 2 x 2688] against npm_scale over a tensor of the same total bytes (12 / 20 bytes per gated
     element against 8 per element of npm_scale), each as a fraction of the 8 TB/s HBM peak.
  3. One TransformerEncoder step (forward + backward + SGD) at bench.py's headline shape (batch 256, seq 512, F 1024, 8 heads, pre-norm):
     the default block (LayerNorm, ReLU, U = 4096) against norm='rms', ffn='swiglu' at equal parameter count (U = 2/3 x 4096 rounded
     to a multiple of 128 = 2688): samples/s, the share of the step in the two swiglu launches (the number a gate folded into the
     GEMM epilogue has to beat) and, for d = 1024, the RMSNorm kernels' time inside the step under both hint placements
     (NPM_TUNE_LN_NT_SPLIT 5: nontemporal loads only, the default; 0: loads and stores).

Cold buffers: every tensor here has at least 512 MB, twice the Infinity Cache, and is walked once per call.  Microseconds per call
from HIP events around a window of back-to-back calls; the variants of a group alternate; median (min .. max) over the windows.

    python tools/llama_block_bench.py > profiles/r23_llama_block_bench.log
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8e12
KNOB_LN_NT_SPLIT = 19


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--calls', type=int, default=6, help='calls per timed window')
    ap.add_argument('--steps', type=int, default=3, help='encoder steps per timed window')
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--skip-encoder', action='store_true')
    a = ap.parse_args()

    import np_modeling_amd as npm
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    print(f'llama_block_bench: sources {_C.source_id()}; {a.windows} windows of {a.calls} calls ({a.steps} encoder steps) per variant, '
          f'alternating, after untimed calls; microseconds per call, median (min .. max)', flush=True)
    rng = np.random.default_rng(0)
    chunk = 1 << 22
    noise = D.from_host((2 * rng.standard_normal(chunk) + 0.5).astype(np.float32))

    def filled(n):
        t = D.empty([n])
        for at in range(0, n, chunk):
            _C.check(lib.npm_d2d(t.ptr + 4 * at, noise.ptr, 4 * min(chunk, n - at)), 'npm_d2d')
        return t

    def window(fn, calls):
        start = D.Event().record()
        for _ in range(calls):
            fn()
        stop = D.Event().record()
        stop.synchronize()
        return start.elapsed_ms(stop) * 1e3 / calls

    def measure(fns, calls):
        for fn in fns:
            fn()
            fn()
        times = {fn: [] for fn in fns}
        for _ in range(a.windows):
            for fn in fns:
                times[fn].append(window(fn, calls))
        return [times[fn] for fn in fns]

    med = lambda ts: sorted(ts)[len(ts) // 2]
    fmt = lambda ts: f'{med(ts):10.1f} ({min(ts):.1f} .. {max(ts):.1f})'
    spread = lambda ts: (max(ts) - min(ts)) / med(ts)

    # ---- 1. RMSNorm against LayerNorm ---------------------------------------------------------------------------------------
    for rows, d in ((131072, 1024), (65536, 4096)):
        n = rows * d
        x, dz, res, out = filled(n), filled(n), filled(n), D.empty([n])
        gamma, beta = filled(d), filled(d)
        mean, rstd, grads = D.empty([rows]), D.empty([rows]), D.empty([2 * d])
        ck = _C.check
        rms_f = lambda: ck(lib.npm_rmsnorm_fwd(x.ptr, gamma.ptr, 1e-6, rows, d, out.ptr, rstd.ptr), 'npm_rmsnorm_fwd')
        ln_f = lambda: ck(lib.npm_layernorm_fwd(x.ptr, gamma.ptr, beta.ptr, 1e-3, rows, d, out.ptr, mean.ptr, rstd.ptr), 'npm_layernorm_fwd')
        t_rf, t_lf = measure([rms_f, ln_f], a.calls)
        rms_f()                                                     # rstd for the RMSNorm backward, then LayerNorm's statistics
        rstd_rms = rstd.copy()
        ln_f()
        rms_b = lambda: ck(lib.npm_rmsnorm_bwd(dz.ptr, x.ptr, rstd_rms.ptr, gamma.ptr, res.ptr, rows, d, out.ptr, grads.ptr), 'npm_rmsnorm_bwd')
        ln_b = lambda: ck(lib.npm_layernorm_bwd(dz.ptr, x.ptr, mean.ptr, rstd.ptr, gamma.ptr, res.ptr, rows, d, out.ptr, grads.ptr,
                                                grads.ptr + 4 * d), 'npm_layernorm_bwd')
        t_rb, t_lb = measure([rms_b, ln_b], a.calls)
        tb = lambda ts, passes: 4.0 * n * passes / (med(ts) * 1e-6) / 1e12
        print(f'\n[{rows}, {d}] ({4 * n / 2 ** 20:.0f} MB per tensor)', flush=True)
        print(f'  npm_rmsnorm_fwd     {fmt(t_rf)}   {tb(t_rf, 2):5.2f} TB/s')
        print(f'  npm_layernorm_fwd   {fmt(t_lf)}   {tb(t_lf, 2):5.2f} TB/s   spread {spread(t_lf):.3f}')
        print(f'  npm_rmsnorm_bwd     {fmt(t_rb)}   {tb(t_rb, 4):5.2f} TB/s   (with a residual: 4 passes)')
        print(f'  npm_layernorm_bwd   {fmt(t_lb)}   {tb(t_lb, 4):5.2f} TB/s   spread {spread(t_lb):.3f}')
        print(f'  rmsnorm / layernorm: forward {med(t_rf) / med(t_lf):.3f}, backward {med(t_rb) / med(t_lb):.3f}', flush=True)
        del x, dz, res, out, rstd_rms
        D.trim_pool()

    # ---- 2. the gate against npm_scale ---------------------------------------------------------------------------------------------
    rows, units = 131072, 2688
    pre, dh = filled(2 * rows * units), filled(rows * units)
    h, dpre = D.empty([rows * units]), D.empty([2 * rows * units])
    gate_f = lambda: _C.check(lib.npm_swiglu_fwd(pre.ptr, 2 * units, rows, units, h.ptr, units), 'npm_swiglu_fwd')
    gate_b = lambda: _C.check(lib.npm_swiglu_bwd(pre.ptr, 2 * units, dh.ptr, units, rows, units, dpre.ptr, 2 * units), 'npm_swiglu_bwd')
    n_f, n_b = 3 * rows * units // 2, 5 * rows * units // 2          # 8 n bytes of npm_scale = 12 / 20 bytes per gated element
    scale_f = lambda: _C.check(lib.npm_scale(pre.ptr, dpre.ptr, 0.5, n_f), 'npm_scale')
    t_gf, t_sf = measure([gate_f, scale_f], a.calls)
    del h
    src = filled(n_b)
    dst = D.empty([n_b])
    scale_b = lambda: _C.check(lib.npm_scale(src.ptr, dst.ptr, 0.5, n_b), 'npm_scale')
    t_gb, t_sb = measure([gate_b, scale_b], a.calls)
    share = lambda ts, nbytes: nbytes / (med(ts) * 1e-6) / PEAK
    print(f'\n[{rows}, 2 x {units}] ({8 * rows * units / 2 ** 20:.0f} MB of pre)', flush=True)
    print(f'  npm_swiglu_fwd      {fmt(t_gf)}   {share(t_gf, 12.0 * rows * units):5.3f} of 8 TB/s')
    print(f'  npm_scale, same B   {fmt(t_sf)}   {share(t_sf, 8.0 * n_f):5.3f} of 8 TB/s   spread {spread(t_sf):.3f}')
    print(f'  npm_swiglu_bwd      {fmt(t_gb)}   {share(t_gb, 20.0 * rows * units):5.3f} of 8 TB/s')
    print(f'  npm_scale, same B   {fmt(t_sb)}   {share(t_sb, 8.0 * n_b):5.3f} of 8 TB/s   spread {spread(t_sb):.3f}')
    print(f'  swiglu / npm_scale: forward {med(t_gf) / med(t_sf):.3f}, backward {med(t_gb) / med(t_sb):.3f}', flush=True)
    del pre, dh, dpre, src, dst
    D.trim_pool()
    if a.skip_encoder:
        return

    # ---- 3. the encoder step ---------------------------------------------------------------------------------------------------------
    batch, seq, feat, heads = a.batch, 512, 1024, 8
    gated_units = int(round(2.0 / 3.0 * 4096 / 128)) * 128
    x = D.from_host(rng.standard_normal((batch, seq, feat), dtype=np.float32))
    dy = D.from_host((0.1 * rng.standard_normal((batch, seq, feat), dtype=np.float32)))

    def make(**keywords):
        np.random.seed(0)
        enc = npm.layers.TransformerEncoder(num_heads=heads, hidden_units=keywords.pop('hidden'), norm_first=True, **keywords)
        enc(x)
        for obj, attr in ((enc._self_attention, '_wq'), (enc._self_attention, '_wk'), (enc._self_attention, '_wv'),
                          (enc._self_attention, '_wo'), (enc._dense1._linear, '_w'), (enc._dense2, '_w')):
            value = obj._param(attr)
            _C.check(lib.npm_scale(value.ptr, value.ptr, float(1.0 / np.sqrt(value.shape[0] if value.ndim == 2 else feat)), value.size), 'npm_scale')
        return enc

    opt = npm.optimizer.SGDOptimizer(1e-4)

    def stepper(enc):
        def step():
            enc(x)
            enc(dy, backprop=True, optimizer_=opt)
        return step

    default, llama = make(hidden=4096), make(hidden=gated_units, norm='rms', ffn='swiglu')
    floats = lambda enc: enc._arena.size
    t_def, t_llama = measure([stepper(default), stepper(llama)], a.steps)
    print(f'\nencoder step, batch {batch} x seq {seq} x F {feat}, {heads} heads, pre-norm (microseconds per step)', flush=True)
    print(f'  default (layer, relu, U 4096; {floats(default)} parameters)        {fmt(t_def)}   {batch / (med(t_def) * 1e-6):8.1f} samples/s   spread {spread(t_def):.3f}')
    print(f'  rms, swiglu (U {gated_units}; {floats(llama)} parameters)             {fmt(t_llama)}   {batch / (med(t_llama) * 1e-6):8.1f} samples/s')
    print(f'  rms swiglu / default: {med(t_llama) / med(t_def):.3f} of the time', flush=True)

    def kernels(enc, steps=3):
        stepper(enc)()
        with D.KernelTimer() as timer:
            for _ in range(steps):
                stepper(enc)()
        return {name: rec['ms'] * 1e3 / steps for name, rec in timer.summary().items()}

    for split, label in ((5, 'nontemporal loads only (default)'), (0, 'nontemporal loads and stores')):
        _C.check(lib.npm_set_tuning(KNOB_LN_NT_SPLIT, split), 'npm_set_tuning')
        runs = [kernels(llama) for _ in range(a.windows)]
        pick = lambda name: [r.get(name, 0.0) for r in runs]
        total = [sum(r.values()) for r in runs]
        gate = [r['swiglu_fwd'] + r['swiglu_bwd'] for r in runs]
        print(f'  NPM_TUNE_LN_NT_SPLIT {split}: {label}; per step, microseconds inside the timed kernels')
        print(f'    rmsnorm_fwd (2 launches) {fmt(pick("rmsnorm_fwd"))}   rmsnorm_bwd (2) {fmt(pick("rmsnorm_bwd"))}   all kernels {fmt(total)}')
        print(f'    swiglu_fwd {fmt(pick("swiglu_fwd"))}   swiglu_bwd {fmt(pick("swiglu_bwd"))}   the two swiglu launches: '
              f'{med(gate) / med(total):.4f} of the step\'s kernel time', flush=True)
    _C.check(lib.npm_set_tuning(KNOB_LN_NT_SPLIT, 5), 'npm_set_tuning')


if __name__ == '__main__':
    main()
