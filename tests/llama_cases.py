"""TEST INFRASTRUCTURE ONLY -- the shapes and runs the rms / swiglu block tests share (tests/test_llama_block_host.py on the host
simulator, tests/test_gpu_llama_block.py on the device).

``default_calls()``: the entry points a default-keyword ``TransformerEncoder`` / ``TransformerDecoder`` calls, in order, for one
forward, one backward and (decoder) two decode steps -- what tests/golden/llama_default_calls.json holds, recorded on the commit
before ``norm=`` / ``ffn=`` existed:

    python tests/llama_cases.py             writes the file (run on the commit whose behaviour is to be kept)
"""

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'llama_default_calls.json')

B, S, SKV, F, HEADS, U = 2, 8, 6, 32, 2, 48
CHUNKS = (5, 1, 1, 1)


def inputs(seed, *shapes):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(np.float32) for s in shapes]


def make(npm, kind, norm_first, seed=0, **keywords):
    """A layer of ``kind`` 'encoder' / 'decoder' (causal) at the shared shape, its parameters drawn from ``seed`` at the first call."""
    np.random.seed(seed)
    if kind == 'encoder':
        return npm.layers.TransformerEncoder(num_heads=HEADS, hidden_units=U, norm_first=norm_first, **keywords)
    return npm.layers.TransformerDecoder(num_heads=HEADS, hidden_units=U, norm_first=norm_first, causal=True, **keywords)


def tame(layer):
    """Every matrix of ``layer`` divided by sqrt(F), written in place (the parameter arena stays what it is): O(1) activations."""
    import llama_reference as LR
    for owner, attribute in LR.parameters(layer).values():
        value = owner._param(attribute)
        if value.ndim > 1:
            value.set(np.asarray(value) / np.sqrt(F))


def parity(got, ref, rel, scaled):
    """The two figures of tests/test_gpu_parity.py as fractions of their bounds: (max |got - ref| / max |ref|) / scaled and the
    largest elementwise relative error over the elements with |ref| >= 0.1 max |ref|, / rel."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    top = np.abs(ref).max()
    err = np.abs(got - ref)
    big = np.abs(ref) >= 0.1 * top
    return float(err.max() / top / scaled), float((err[big] / np.abs(ref[big])).max() / rel)


LR_STEP = 0.05


def run_block(npm, kind, norm_first, *, literal=False, norm='rms', ffn='swiglu', drop=0.0, seed=3):
    """One forward, one backward with SGD(LR_STEP) of a tamed layer at the shared shape, in the fused composition or
    (``literal``) the literal one, and the float64 restatement on the same parameters, inputs and dropout masks.  Returns a dict:
    layer, out / dx / dkv / params (the device's, as float32 arrays; dkv None for an encoder), ref_out / ref_dx / ref_dkv /
    ref_params (float64; the parameters after the same step), start (the parameters before it), scope (GradScope.last)."""
    import llama_reference as LR
    from np_modeling_amd import parallel
    D = npm.device
    layer = make(npm, kind, norm_first, seed=seed, norm=norm, ffn=ffn, drop_rate=drop)
    x, kv, dy = inputs(seed + 1, [B, S, F], [B, SKV, F], [B, S, F])
    args = (x,) if kind == 'encoder' else (x, kv)
    layer(*args)                                    # parameters
    tame(layer)
    start = LR.values(layer)
    opt = npm.optimizer.SGDOptimizer(LR_STEP)
    if literal:
        out = np.asarray(layer._forward_unfused(*(D.as_device(a) for a in args)))
    else:
        out = np.asarray(layer(*args))
    masks = None
    if drop:
        masks = [np.asarray(d._mask) for d in (layer._dropout1, layer._dropout2, getattr(layer, '_dropout3', None)) if d is not None]
    if literal:
        with parallel.grad_scope(layer._numel(), layer._arena) as scope:
            grads = layer._backward_unfused(D.as_device(dy), opt, scope)
    else:
        grads = layer(dy, backprop=True, optimizer_=opt)
    dx, dkv = (grads if isinstance(grads, tuple) else (grads, None))
    ref_out, backward = LR.block_forward(start, x, kv if kind == 'decoder' else None, norm_first=norm_first, norm=norm, ffn=ffn,
                                         causal=kind == 'decoder', masks=masks, keep=1.0 - drop)
    ref_dx, ref_dkv, ref_grads = backward(dy)
    return dict(layer=layer, out=out, dx=np.asarray(dx), dkv=None if dkv is None else np.asarray(dkv), params=LR.values(layer),
                ref_out=ref_out, ref_dx=ref_dx, ref_dkv=ref_dkv, start=start, ref_grads=ref_grads,
                ref_params={k: start[k] - LR_STEP * ref_grads[k] for k in start}, scope=dict(parallel.GradScope.last))


def default_calls():
    """{'encoder pre': {'forward': [...], 'backward': [...]}, ..., 'decoder post': {..., 'decode 5': [...], 'decode 1': [...]}} on a
    fresh host simulator behind tests/transformer_trace_cases.py's Recorder."""
    import transformer_trace_cases as TC
    from hostsim.fixtures import activate, deactivate
    from np_modeling_amd import _C
    out = {}
    for kind in ('encoder', 'decoder'):
        for norm_first in (True, False):
            npm = activate()
            try:
                recorder = TC.Recorder(npm.sim)
                _C._LIB = recorder
                seen = [0]

                def phase():
                    names = [r[0] for r in recorder.records[seen[0]:]]
                    seen[0] = len(recorder.records)
                    return names

                layer = make(npm, kind, norm_first, seed=11)
                x, kv, dy = inputs(5, [B, S, F], [B, SKV, F], [B, S, F])
                args = (x,) if kind == 'encoder' else (x, kv)
                trace = {}
                layer(*args)
                trace['forward'] = phase()
                layer(dy, backprop=True, optimizer_=npm.optimizer.SGDOptimizer(0.05))
                trace['backward'] = phase()
                if kind == 'decoder':
                    state = layer.start_decoding(kv, 16)
                    trace['start_decoding'] = phase()
                    layer.decode(x[:, :5], state)
                    trace['decode 5'] = phase()
                    layer.decode(x[:, 5:6], state)
                    trace['decode 1'] = phase()
                out[f'{kind} {"pre" if norm_first else "post"}'] = trace
            finally:
                deactivate()
    return out


if __name__ == '__main__':
    sys.path[:0] = [HERE, os.path.dirname(HERE)]
    with open(GOLDEN, 'w') as f:
        json.dump(default_calls(), f, indent=0, sort_keys=True)
        f.write('\n')
    print('wrote', GOLDEN, os.path.getsize(GOLDEN), 'bytes')
