"""TEST INFRASTRUCTURE ONLY -- what the transformer layers and ``MultiHeadAttention`` ASK of the library, scenario by scenario.

``SCENARIOS`` names small runs (F 64, 4 heads, hidden 48, B 2, Sq 5, Skv 7) that take every branch of layers/transformer.py and the
projection / composition branches of layers/attentions.py.  ``run(name)`` runs one on the host simulator behind a ``Recorder`` and
returns what tests/golden/transformer_traces.json stores for it:

* ``phases``   per phase (forward, backward, one decode step, ...) the entry points called, in order, and the sha256 of the full
               call records; ``KEEP_RECORDS`` (decoding, contiguous and paged) also keep the records themselves.  A record is the name and every argument:
               integers, floats and flags as they are, a descriptor struct field by field, and of every pointer (argument or
               field) only whether it is null -- allocation order and pool reuse may change, so no address is recorded.  The
               runtime (memory, copies, events, knobs: hostsim/runtime.py) is not recorded for the same reason
* ``uploads``  the byte counts of the host-to-device copies
* ``tensors``  sha256 of every returned tensor; ``params``: sha256 of every parameter at the end (after the update, if any)
* ``arena``    the layer's parameters as (path, attribute, offset) in ``ParamArena`` order, where ``offset_of`` still finds them
* ``collectives`` / ``flushed``  ``GradScope.collectives`` and the (offset, size) ranges of the bucket handed to a recording
               two-rank transport, per backward
* ``took``     what the run observed of the layers afterwards (composition, norm order, cached path, packed projection): the
               coverage test of tests/test_transformer_trace_host.py reads it

The simulator is deterministic NumPy, so equality is bitwise.

    python tests/transformer_trace_cases.py             writes tests/golden/transformer_traces.json (run on the commit whose
                                                         behaviour is to be kept, not after a refactor)
    python tests/transformer_trace_cases.py --digest    one sha256 line per scenario from the REAL library on the device
"""

import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'transformer_traces.json')

F, HEADS, HIDDEN, B, SQ, SKV = 64, 4, 48, 2, 5, 7
PARAM_NAMES = ('_w', '_b', '_wq', '_wk', '_wv', '_wo', '_bq', '_bk', '_bv', '_bo', '_gamma', '_beta')


def _sha(array) -> str:
    a = np.ascontiguousarray(np.asarray(array))
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


# -- the recorder ---------------------------------------------------------------------------------------------------------------
def _null(p) -> str:
    if p is None:
        return 'null'
    v = p if isinstance(p, int) else getattr(p, 'value', None)
    return 'ptr' if v else 'null'


def _scalar(v):
    v = getattr(v, 'value', v)
    if isinstance(v, bytes):
        return v.decode()
    return float(v) if isinstance(v, float) else int(v)


def _encode(arg, argtype):
    if argtype is C.c_void_p:
        return _null(arg)
    if isinstance(argtype, type) and issubclass(argtype, C._Pointer):
        target = argtype._type_
        if issubclass(target, C.Structure):
            struct = arg._obj if hasattr(arg, '_obj') else arg
            return [_null(getattr(struct, f)) if t is C.c_void_p else _scalar(getattr(struct, f)) for f, t in target._fields_]
        return 'out'                                          # a scalar result written through the pointer
    return _scalar(arg)


class Recorder:
    """A proxy in front of an installed simulator, by composition: the simulator gains nothing.
    Every attribute is the simulator's; an entry point that is not part of the runtime is also recorded when called."""

    def __init__(self, sim):
        from hostsim.runtime import Runtime
        from np_modeling_amd import _C
        self.sim = sim
        self.records = []
        self._signatures = dict(_C.SIGNATURES, **{name: types for name, (_, types) in _C._SPECIAL.items()})
        self._runtime = frozenset(n for n in vars(Runtime) if n.startswith('npm_'))

    def __getattr__(self, name):                # only what this class does not define
        attr = getattr(self.sim, name)
        if not name.startswith('npm_') or name in self._runtime:
            return attr
        types = self._signatures[name]

        def entry(*args):
            assert len(args) == len(types), name
            self.records.append([name] + [_encode(a, t) for a, t in zip(args, types)])
            return attr(*args)
        return entry


class _TwoRanks:
    """A transport of two ranks that moves nothing and notes which ranges (of the one gradient bucket) it was handed."""
    rank, world_size, active = 0, 2, True

    def __init__(self):
        self.sent = []

    def allreduce_async(self, flat, op):
        self.sent.append((flat.ptr, int(flat.size)))

    def wait(self):
        pass


class Run:
    """One scenario's bookkeeping: phases of calls, tensors, backward exchanges, observations."""

    def __init__(self, npm, recorder=None, comm=None, keep_records=False):
        self.npm, self.recorder, self.comm, self.keep = npm, recorder, comm, keep_records
        self.out = {'phases': [], 'tensors': {}, 'collectives': [], 'flushed': [], 'took': []}
        self._seen = 0

    def phase(self, label):
        """Everything called since the last phase ended belongs to ``label``."""
        if self.recorder is None:
            return
        records = self.recorder.records[self._seen:]
        self._seen = len(self.recorder.records)
        entry = {'label': label, 'calls': [r[0] for r in records],
                 'sha256': hashlib.sha256(json.dumps(records).encode()).hexdigest()}
        if self.keep:
            entry['records'] = [json.dumps(r, separators=(',', ':')) for r in records]
        self.out['phases'].append(entry)

    def tensor(self, label, value):
        self.out['tensors'][label] = _sha(value)
        return value

    def backward(self, label, call):
        """``call()`` is a backward: its tensors, its phase, and what its outermost GradScope exchanged."""
        from np_modeling_amd import parallel
        if self.comm is not None:
            self.comm.sent.clear()
        result = call()
        for i, g in enumerate(result if isinstance(result, tuple) else (result,)):
            self.tensor(f'{label}.{i}', g)
        self.phase(label)
        if self.comm is not None:
            self.out['collectives'].append(parallel.GradScope.last['collectives'])
            first = min(ptr for ptr, _ in self.comm.sent)              # offsets within the one bucket, not addresses
            self.out['flushed'].append([[(ptr - first) // 4, size] for ptr, size in self.comm.sent])
        return result

    def took(self, *tags):
        self.out['took'] += [t for t in tags if t not in self.out['took']]

    def finish(self, layer):
        found, stack, seen = {}, [('', layer)], set()
        while stack:
            path, obj = stack.pop()
            if id(obj) in seen:
                continue
            seen.add(id(obj))
            for key in sorted(vars(obj)):
                value = getattr(obj, key)
                if key in PARAM_NAMES and value is not None:
                    found[id(obj), key] = f'{path}{key}'
                    self.out.setdefault('params', {})[f'{path}{key}'] = _sha(obj._param(key))
                elif isinstance(value, self.npm.layers.layer.Layer):
                    stack.append((f'{path}{key}.', value))
        arena = layer._arena
        self.out['arena'] = [] if arena is None else [
            [found.get((id(ref()), a), '?'), arena.offset_of(ref(), a, n)] for ref, a, off, n in arena.entries]
        if self.recorder is not None:
            self.out['uploads'] = list(self.recorder.sim.uploads)
        return self.out


# -- scenarios ------------------------------------------------------------------------------------------------------------------
def _inputs(seed, *shapes):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(np.float32) for s in shapes]


def _scope(layer):
    from np_modeling_amd import parallel
    return parallel.grad_scope(layer._numel(), layer._arena)


def _composition(run, kind, layer):
    run.took(f'{kind} {"pre" if layer._norm_first else "post"} {"fused" if layer._fused else "unfused"}')
    att = layer._self_attention
    run.took('packed' if att._packed else 'unpacked')


def encoder(run, seed, norm_first, drop, kv_heads, adam=False, unfused=False):
    npm = run.npm
    np.random.seed(seed)
    enc = npm.layers.TransformerEncoder(num_heads=HEADS, hidden_units=HIDDEN, norm_first=norm_first, drop_rate=drop,
                                        num_kv_heads=kv_heads)
    x, dy = _inputs(seed, [B, SQ, F], [B, SQ, F])
    opt = npm.optimizer.AdamOptimizer(0.01) if adam else npm.optimizer.SGDOptimizer(0.05)
    run.tensor('out', enc(x))
    run.phase('forward')
    if unfused:
        run.tensor('out_unfused', enc._forward_unfused(npm.device.as_device(x)))
        run.phase('forward_unfused')

        def backward():
            with _scope(enc) as scope:
                return enc._backward_unfused(npm.device.as_device(dy), opt, scope)
        run.backward('backward_unfused', backward)
        run.took(f'encoder {"pre" if norm_first else "post"} unfused')
    else:
        run.backward('backward', lambda: enc(dy, backprop=True, optimizer_=opt))
        _composition(run, 'encoder', enc)
        run.tensor('out2', enc(x))                       # the updated parameters at work
        run.phase('forward2')
        if adam:
            run.backward('backward2', lambda: enc(dy, backprop=True, optimizer_=opt))
    return enc


def decoder(run, seed, norm_first, drop, causal, kv_heads, window=None, rope=None, unfused=False):
    npm = run.npm
    np.random.seed(seed)
    dec = npm.layers.TransformerDecoder(num_heads=HEADS, hidden_units=HIDDEN, norm_first=norm_first, drop_rate=drop,
                                        num_kv_heads=kv_heads, causal=causal, window=window, rope_base=rope)
    q, kv, dy = _inputs(seed, [B, SQ, F], [B, SKV, F], [B, SQ, F])
    opt = npm.optimizer.SGDOptimizer(0.05)
    run.tensor('out', dec(q, kv))
    run.phase('forward')
    if unfused:
        as_device = npm.device.as_device
        run.tensor('out_unfused', dec._forward_unfused(as_device(q), as_device(kv)))
        run.phase('forward_unfused')

        def backward():
            with _scope(dec) as scope:
                return dec._backward_unfused(as_device(dy), opt, scope)
        run.backward('backward_unfused', backward)
        run.took(f'decoder {"pre" if norm_first else "post"} unfused')
    else:
        run.backward('backward', lambda: dec(dy, backprop=True, optimizer_=opt))
        _composition(run, 'decoder', dec)
        run.tensor('out2', dec(q, kv))
        run.phase('forward2')
    return dec


def decoding(run, seed, norm_first, kv_heads, paged=False, weights=None, cache_dtype='f32', rope=None):
    npm = run.npm
    np.random.seed(seed)
    dec = npm.layers.TransformerDecoder(num_heads=HEADS, hidden_units=HIDDEN, norm_first=norm_first, num_kv_heads=kv_heads,
                                        causal=True, rope_base=rope)
    q, kv, chunk, tok1, tok2, tok3, kv_new, tok4 = _inputs(seed, [B, 2, F], [B, SKV, F], [B, 3, F], [B, 1, F], [B, 1, F], [B, 1, F],
                                                          [1, 6, F], [B, 2, F])
    dec(q, kv)                                           # parameters
    run.phase('forward')
    state = dec.start_decoding(kv, 32, kv_lengths=[SKV, 4] if paged else None, weights=weights, cache_dtype=cache_dtype,
                               **(dict(page_size=16, memory_capacity=8) if paged else {}))
    run.phase('start_decoding')

    def step(label, x, n=None):
        run.tensor(label, dec.decode(x, state, new_lengths=n))
        run.phase(label)
        run.took('self ' + dec._self_attention._cached_path, 'cross ' + dec._cross_attention._cached_path)

    step('chunk T=3', chunk)
    step('step 1', tok1)
    step('step 2', tok2)
    step('ragged [1, 0]', tok3, [1, 0])
    if paged:
        state.release(1)
        run.phase('release(1)')
        dec.admit(state, 1, kv_new, kv_length=5)
        run.phase('admit(1)')
        step('re-admitted [1, 2]', tok4, [1, 2])
    run.out['tensors']['lengths'] = [state.self_cache.lengths.tolist(), state.cross_cache.lengths.tolist()]
    return dec


class _Gradients:
    """An optimizer that notes the gradients' digests and updates nothing."""

    def __init__(self, run):
        self.run = run

    def update(self, obj, attribute, gradient):
        self.run.tensor('gradient' + attribute, gradient)


def attention(run, seed, kv_heads, cross=False, features=F, rebind=False):
    npm = run.npm
    np.random.seed(seed)
    att = npm.layers.MultiHeadAttention(HEADS, num_kv_heads=kv_heads)
    x, kv, dy = _inputs(seed, [B, SQ, features], [B, SKV, features], [B, SQ, features])
    args = (x, kv, kv) if cross else (x,)
    run.tensor('out', att(*args))
    run.phase('forward')
    run.took('packed' if att._packed else 'unpacked', 'core' if att._core else 'gemm composition')
    optimizer = npm.optimizer.SGDOptimizer(0.05)
    if rebind:
        # a weight binder between forward and backward: no longer adjacent.  The gradients are recorded instead of applied: the
        # update queue walks loose parameters in address order, which is not this trace's business
        att._wk = np.asarray(att._wk).copy()
        optimizer = _Gradients(run)
    run.backward('backward', lambda: att(dy, backprop=True, optimizer_=optimizer))
    run.tensor('out2', att(*args))
    run.phase('forward2')
    run.took('packed' if att._packed else 'unpacked')
    return att


def attention_cached(run, seed, kv_heads, features, cross, lengths=None, last=3):
    """``fill_cache`` (with ``lengths``) and a frozen forward, or (``cross`` False) a growing cache in chunks of 3, 1 and ``last``."""
    npm = run.npm
    np.random.seed(seed)
    att = npm.layers.MultiHeadAttention(HEADS, num_kv_heads=kv_heads)
    x, kv, chunk, tok, chunk2 = _inputs(seed, [B, 2, features], [B, SKV, features], [B, 3, features], [B, 1, features],
                                        [B, last, features])
    att(x)
    run.phase('forward')
    cache = att.make_cache(B, 32)
    pieces = [('chunk T=3', chunk), ('step', tok), (f'chunk T={last}', chunk2)]
    if cross:
        att.fill_cache(cache, kv, lengths=lengths)
        run.phase('fill_cache')
        pieces = pieces[:2]
    for label, piece in pieces:
        run.tensor(label, att(piece, cache=cache))
        run.phase(label)
        run.took('path ' + att._cached_path)
    run.out['tensors']['lengths'] = cache.lengths.tolist()
    return att


def _scenarios():
    table, seed = {}, 100
    for pre in (True, False):
        order = 'pre' if pre else 'post'
        for drop in (0.0, 0.1):
            seed += 1
            table[f'encoder {order} drop {drop}'] = (encoder, dict(seed=seed, norm_first=pre, drop=drop, kv_heads=4 if drop else 2))
        seed += 1
        table[f'encoder {order} unfused'] = (encoder, dict(seed=seed, norm_first=pre, drop=0.0, kv_heads=4, unfused=True))
    table['encoder pre adam'] = (encoder, dict(seed=120, norm_first=True, drop=0.0, kv_heads=4, adam=True))
    seed = 200
    for pre in (True, False):
        order = 'pre' if pre else 'post'
        for drop in (0.0, 0.1):
            for causal in (False, True):
                seed += 1
                table[f'decoder {order} drop {drop}{" causal" if causal else ""}'] = (
                    decoder, dict(seed=seed, norm_first=pre, drop=drop, causal=causal, kv_heads=2 if causal else 4))
        for causal in (False, True):
            seed += 1
            table[f'decoder {order} unfused{" causal" if causal else ""}'] = (
                decoder, dict(seed=seed, norm_first=pre, drop=0.0, causal=causal, kv_heads=4, unfused=True))
    table['decoder pre window 3'] = (decoder, dict(seed=230, norm_first=True, drop=0.0, causal=True, kv_heads=2, window=3))
    table['decoder post rope'] = (decoder, dict(seed=231, norm_first=False, drop=0.0, causal=True, kv_heads=4, rope=10000.0))
    seed = 300
    for pre in (True, False):
        order = 'pre' if pre else 'post'
        for label, extra in (('contiguous', {}), ('paged', dict(paged=True)), ('weights f16', dict(weights='f16')),
                             ('cache f16', dict(cache_dtype='f16'))):
            seed += 1
            table[f'decoding {order} {label}'] = (decoding, dict(seed=seed, norm_first=pre, kv_heads=2 if pre else 4, **extra))
    table['decoding pre rope'] = (decoding, dict(seed=320, norm_first=True, kv_heads=2, rope=10000.0))
    table['attention self'] = (attention, dict(seed=401, kv_heads=4))
    table['attention self grouped'] = (attention, dict(seed=402, kv_heads=2))
    table['attention cross'] = (attention, dict(seed=403, kv_heads=2, cross=True))
    table['attention self Dk 24'] = (attention, dict(seed=404, kv_heads=4, features=96))
    table['attention self grouped Dk 24'] = (attention, dict(seed=405, kv_heads=2, features=96))
    table['attention cross Dk 24'] = (attention, dict(seed=406, kv_heads=4, features=96, cross=True))
    table['attention self rebound'] = (attention, dict(seed=407, kv_heads=2, rebind=True))
    table['attention fill_cache lengths'] = (attention_cached, dict(seed=408, kv_heads=2, features=F, cross=True, lengths=[SKV, 3]))
    table['attention cached Dk 24'] = (attention_cached, dict(seed=409, kv_heads=2, features=96, cross=False))
    table['attention cached Dk 24 frozen'] = (attention_cached, dict(seed=410, kv_heads=4, features=96, cross=True))
    # 2 x 17 = 34 score rows per K / V head: more than the decode kernel takes, so the fused forward with a mask
    table['attention cached chunk 17'] = (attention_cached, dict(seed=411, kv_heads=2, features=F, cross=False, last=17))
    return table


SCENARIOS = _scenarios()
KEEP_RECORDS = ('decoding pre contiguous', 'decoding post contiguous', 'decoding pre paged', 'decoding post paged')


def run(name):
    """Scenario ``name`` on a fresh simulator behind a Recorder, with the recording two-rank transport."""
    from hostsim.fixtures import activate, deactivate
    from np_modeling_amd import _C, parallel
    function, arguments = SCENARIOS[name]
    npm = activate()
    try:
        recorder = Recorder(npm.sim)
        _C._LIB = recorder
        comm = _TwoRanks()
        parallel.set_communicator(comm)
        trace = Run(npm, recorder, comm, keep_records=name in KEEP_RECORDS)
        return trace.finish(function(trace, **arguments))
    finally:
        deactivate()


def digest(name):
    """Scenario ``name`` on the real library: one sha256 over every returned tensor and every parameter at the end."""
    import np_modeling_amd as npm
    function, arguments = SCENARIOS[name]
    trace = Run(npm)
    out = trace.finish(function(trace, **arguments))
    return hashlib.sha256(json.dumps([out['tensors'], out['params']], sort_keys=True).encode()).hexdigest()


if __name__ == '__main__':
    sys.path[:0] = [HERE, os.path.dirname(HERE)]
    if '--digest' in sys.argv:
        for scenario in SCENARIOS:
            print(digest(scenario), scenario, flush=True)
    else:
        with open(GOLDEN, 'w') as f:
            json.dump({scenario: run(scenario) for scenario in SCENARIOS}, f, indent=0, sort_keys=True)
            f.write('\n')
        print('wrote', GOLDEN, os.path.getsize(GOLDEN), 'bytes')
