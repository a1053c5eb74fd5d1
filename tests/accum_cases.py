"""TEST INFRASTRUCTURE: the cases and checks of npm_accumulate_ranges and npm_clip_finish_scaled (csrc/npm_accum.hip), of
``optimizer.AdamWOptimizer(accumulate=True)`` and of ``train.Trainer.train(..., micro_batches=k)``, written once and run through
whatever library ``np_modeling_amd._C`` holds: tests/accum_sim.py in tests/test_accum_host.py, libnpm_hip.so in
tests/test_gpu_accum.py.  Models and bounds: tests/accum_reference.py, tests/adamw_reference.py.  Buffers with sentinel guards:
tests/optim_cases.py ``F32`` / ``Raw``.

Sizes come from the launch code: a tile is 16384 elements (one below, one, one above, two and a bit: more than one block, a short last
tile); 1, 3, 4 and 5 elements leave no, or exactly one, aligned group of four at some phase; 255 and 1024 end inside the first trip of
the lanes.  No check of the kernels has a tolerance."""

from __future__ import annotations

import contextlib
import ctypes as C
import io

import numpy as np

import accum_reference as XR
import adamw_cases as AC
import adamw_reference as AR
import lm_cases as MC
import optim_cases as OC
import optim_reference as R

TILE = XR.TILE
BAD_ARGUMENT = OC.BAD_ARGUMENT
LENGTHS = [1, 3, 4, 5, 255, 1024, TILE - 1, TILE, TILE + 1, 2 * TILE + 7]
PHASES = [0, 1, 2, 3]                      # floats behind a 16-byte boundary
DATA = ['normal', 'special']
START = 0.37                               # what *sumsq_acc holds before a call: not zero
SCALES = [1.0 / 3.0, 1.0 / 14.0]


def _lib():
    from np_modeling_amd import _C
    return _C, _C.lib()


def fold_data(kind: str, n: int, rng):
    """(a, b).  'special': +-0, subnormals, +-inf and NaN among N(0, 1).  An inf meets a finite value or an inf of its own sign and
    a NaN (the canonical quiet one) meets a finite value: IEEE 754 leaves the sign and payload of a NaN that an operation MAKES
    (inf - inf) to the implementation, the bits of one that is handed through are the operand's."""
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    if kind == 'special' and n:
        tiny = np.float32(1e-40)
        pool = [(0.0, -0.0), (-0.0, -0.0), (-0.0, 0.0), (tiny, tiny), (-tiny, np.float32(3e-41)), (tiny, -tiny), (np.inf, 1.0),
                (-np.inf, -np.inf), (2.0, np.inf), (np.nan, 1.0), (-3.0, np.nan), (np.float32(1.1754944e-38), -tiny)]
        where = rng.permutation(n)[:max(1, n // 3)]
        for k, i in enumerate(where):
            a[i], b[i] = pool[k % len(pool)]
    return a, b


def at_phase(npm, n, phase, host):
    buf = OC.F32(npm, n, phase, host if n else None)
    assert (buf.ptr // 4) % 4 == phase or n == 0, 'a device array does not start on a 16-byte boundary'
    return buf


def tables(pairs):
    """Two npm_ranges from [(dst address, src address, n), ...]."""
    dst = AC.ranges_table([(d, n) for d, _, n in pairs])
    src = AC.ranges_table([(s, n) for _, s, n in pairs])
    return dst, src


def accumulate(pairs, acc=None) -> int:
    _C, lib = _lib()
    dst, src = tables(pairs)
    return lib.npm_accumulate_ranges(C.byref(dst), C.byref(src), None if acc is None else acc.ptr)


def _acc(npm, value=START):
    return OC.Raw(npm, np.float64, 1, 8, np.array([value]))


def _sumsq_bits(npm, parts) -> int:
    """The 8 bytes npm_sumsq_ranges leaves in an accumulator that starts at START."""
    acc = _acc(npm)
    AC.sumsq(npm, parts, acc)
    assert acc.guards_intact()
    return int(R.bits(acc.numpy())[0])


def check_fold_single(npm, kind: str) -> int:
    """One pair of every length at every dst phase x src phase: the plain call, then the fused call on restored inputs, twice.
    Returns the number of cells run."""
    _C, lib = _lib()
    cells = 0
    for n in LENGTHS:
        for dp in PHASES:
            for sp in PHASES:
                rng = np.random.default_rng(100000 + 16 * n + 4 * dp + sp)
                a, b = fold_data(kind, n, rng)
                with np.errstate(all='ignore'):
                    want = a + b
                dst, src = at_phase(npm, n, dp, a), at_phase(npm, n, sp, b)
                what = f'{kind} n={n} dst phase {dp} src phase {sp}'
                _C.check(accumulate([(dst.ptr, src.ptr, n)]), 'npm_accumulate_ranges')
                got = dst.numpy()
                assert np.array_equal(R.bits(got), R.bits(want)), \
                    f'{what}: {int((R.bits(got) != R.bits(want)).sum())} elements differ from float32 a + b'
                assert dst.guards_intact() and src.guards_intact(), f'{what}: a guard was written'
                assert np.array_equal(R.bits(src.numpy()), R.bits(b)), f'{what}: src was written'
                seen = []
                for _ in range(2):                       # restored inputs, the sum in the same pass: the same bits, twice
                    dst.view.set(a)
                    acc = _acc(npm)
                    _C.check(accumulate([(dst.ptr, src.ptr, n)], acc), 'npm_accumulate_ranges')
                    assert np.array_equal(R.bits(dst.numpy()), R.bits(want)), f'{what}: the fused call folds differently'
                    assert acc.guards_intact() and dst.guards_intact() and src.guards_intact(), f'{what}: a guard was written'
                    seen.append(int(R.bits(acc.numpy())[0]))
                assert seen[0] == seen[1], f'{what}: a repeated call differs'
                assert seen[0] == _sumsq_bits(npm, [(dst.ptr, n)]), f'{what}: not the bits of npm_sumsq_ranges on the updated dst'
                cells += 1
    return cells


TABLES = {                                              # name -> lengths; phases cycle, a zero-length range among them
    '1 range': [TILE + 3],
    '5 ranges': [TILE + 3, 0, 5, 2 * TILE, 257],
    '32 ranges': [0 if i == 7 else 1 + 37 * i for i in range(32)],
}


def _table_buffers(npm, sizes, rng):
    data = [fold_data('normal', n, rng) for n in sizes]
    dsts = [at_phase(npm, n, i % 4, a) for i, (n, (a, _)) in enumerate(zip(sizes, data))]
    srcs = [at_phase(npm, n, (3 * i + 1) % 4, b) for i, (n, (_, b)) in enumerate(zip(sizes, data))]
    return data, dsts, srcs


def check_fold_tables(npm) -> None:
    """1, 5 and 32 pairs in one call, a zero-length one (with NULL addresses) among them; count == 0; every table also with the
    sum in the same pass against npm_sumsq_ranges over the same table."""
    _C, lib = _lib()
    for name, sizes in TABLES.items():
        rng = np.random.default_rng(len(sizes))
        data, dsts, srcs = _table_buffers(npm, sizes, rng)
        pairs = [(d.ptr, s.ptr, n) if n else (None, None, 0) for d, s, n in zip(dsts, srcs, sizes)]
        _C.check(accumulate(pairs), 'npm_accumulate_ranges')
        for (a, b), d, s in zip(data, dsts, srcs):
            assert np.array_equal(R.bits(d.numpy()), R.bits(a + b)), name
            assert np.array_equal(R.bits(s.numpy()), R.bits(b)), f'{name}: src was written'
            assert d.guards_intact() and s.guards_intact(), f'{name}: a word before, between or behind the ranges was written'
        seen = []
        for _ in range(2):
            for (a, _), d in zip(data, dsts):
                if d.n:
                    d.view.set(a)
            acc = _acc(npm)
            _C.check(accumulate(pairs, acc), 'npm_accumulate_ranges')
            seen.append(int(R.bits(acc.numpy())[0]))
            assert acc.guards_intact()
        for (a, b), d in zip(data, dsts):
            assert np.array_equal(R.bits(d.numpy()), R.bits(a + b)) and d.guards_intact(), name
        assert seen[0] == seen[1], f'{name}: a repeated call differs'
        assert seen[0] == _sumsq_bits(npm, [(p[0], p[2]) for p in pairs]), f'{name}: not the bits of npm_sumsq_ranges'
    acc = _acc(npm)
    assert accumulate([]) == 0 and accumulate([], acc) == 0 and accumulate([(None, None, 0)], acc) == 0
    assert acc.numpy()[0] == START and acc.guards_intact()


def check_fold_split_32_plus_1(npm) -> None:
    """33 pairs as two calls onto one accumulator against npm_sumsq_ranges called the same way."""
    _C, lib = _lib()
    sizes = [5 + i for i in range(33)]
    data, dsts, srcs = _table_buffers(npm, sizes, np.random.default_rng(33))
    pairs = [(d.ptr, s.ptr, n) for d, s, n in zip(dsts, srcs, sizes)]
    acc = _acc(npm)
    _C.check(accumulate(pairs[:32], acc), 'npm_accumulate_ranges')
    _C.check(accumulate(pairs[32:], acc), 'npm_accumulate_ranges')
    want = _acc(npm)
    AC.sumsq(npm, [(d, n) for d, _, n in pairs[:32]], want)
    AC.sumsq(npm, [(d, n) for d, _, n in pairs[32:]], want)
    assert R.bits(acc.numpy())[0] == R.bits(want.numpy())[0]
    for (a, b), d in zip(data, dsts):
        assert np.array_equal(R.bits(d.numpy()), R.bits(a + b)) and d.guards_intact()


def check_fold_refusals(npm) -> None:
    """Every refusal of the header, each leaving dst (and the accumulator) as they were."""
    _C, lib = _lib()
    ones = np.ones(16, dtype=np.float32)
    dst, other, src = OC.F32(npm, 16, 0, ones), OC.F32(npm, 16, 0, ones), OC.F32(npm, 16, 0, 2 * ones)
    acc = _acc(npm)
    good = [(dst.ptr, src.ptr, 8)]

    def call(d, s, with_acc=True):
        return lib.npm_accumulate_ranges(None if d is None else C.byref(d), None if s is None else C.byref(s), acc.ptr if with_acc else None)

    d, s = tables(good)
    for count in (-1, 33):
        d.count = s.count = count
        assert call(d, s) == BAD_ARGUMENT, f'count {count}'
    d, s = tables(good + [(other.ptr, src.ptr + 32, 8)])
    s.count = 1
    assert call(d, s) == BAD_ARGUMENT, 'dst->count != src->count'
    d, s = tables(good)
    s.n[0] = 7
    assert call(d, s) == BAD_ARGUMENT, 'dst->n != src->n'
    for pair in ((None, src.ptr, 8), (dst.ptr, None, 8)):
        assert call(*tables([pair])) == BAD_ARGUMENT, 'a NULL pointer with n > 0'
    for pair in ((dst.ptr + 2, src.ptr, 8), (dst.ptr, src.ptr + 1, 8)):
        assert call(*tables([pair])) == BAD_ARGUMENT, 'a pointer that is not 4-byte aligned'
    overlaps = {
        'dst over dst': [(dst.ptr, src.ptr, 8), (dst.ptr + 28, src.ptr + 32, 8)],
        'dst over its own src': [(dst.ptr, dst.ptr + 16, 8)],
        'dst over another src': [(dst.ptr, src.ptr, 8), (other.ptr, dst.ptr + 28, 8)],
        'dst is src': [(dst.ptr, dst.ptr, 8)],
    }
    for name, pairs in overlaps.items():
        assert call(*tables(pairs)) == BAD_ARGUMENT, name
        assert call(*tables(pairs), with_acc=False) == BAD_ARGUMENT, name
    assert call(None, tables(good)[1]) == BAD_ARGUMENT and call(tables(good)[0], None) == BAD_ARGUMENT
    for buf, value in ((dst, ones), (other, ones), (src, 2 * ones)):
        assert np.array_equal(buf.numpy(), value) and buf.guards_intact(), 'a refused call wrote something'
    assert acc.numpy()[0] == START and acc.guards_intact()
    # neighbours that only touch are no overlap
    assert call(*tables([(dst.ptr, src.ptr, 8), (dst.ptr + 32, src.ptr + 32, 8)])) == 0
    assert np.array_equal(dst.numpy(), 3 * ones)


# ---- the scaled clip factor -----------------------------------------------------------------------------------------------------------
def check_clip_finish_scaled(npm) -> None:
    """grad_scale 1.0: the four doubles of npm_clip_finish over adamw_cases' cases, the non-finite ones included.  1/3 and 1/14,
    max_norm finite and inf: the NumPy expression, bit for bit."""
    _C, lib = _lib()
    for sumsq_, max_norm in AC.CLIP_CASES:
        start = np.array([sumsq_, -1.0, -1.0, -1.0])
        plain, scaled = OC.Raw(npm, np.float64, 4, 8, start), OC.Raw(npm, np.float64, 4, 8, start)
        _C.check(lib.npm_clip_finish(plain.ptr, max_norm), 'npm_clip_finish')
        _C.check(lib.npm_clip_finish_scaled(scaled.ptr, max_norm, 1.0), 'npm_clip_finish_scaled')
        a, b = plain.numpy(), scaled.numpy()
        same = R.bits(a) == R.bits(b)
        assert (same | (np.isnan(a) & np.isnan(b))).all(), (sumsq_, max_norm, a, b)
        assert scaled.guards_intact()
    for scale in SCALES:
        for sumsq_, max_norm in AC.CLIP_CASES + [(s, float('inf')) for s, _ in AC.CLIP_CASES]:
            state = OC.Raw(npm, np.float64, 4, 8, np.array([sumsq_, -1.0, -1.0, -1.0]))
            _C.check(lib.npm_clip_finish_scaled(state.ptr, max_norm, scale), 'npm_clip_finish_scaled')
            got = state.numpy()
            want = np.array([sumsq_, *XR.clip_finish_scaled(sumsq_, max_norm, scale)])
            assert np.array_equal(R.bits(got), R.bits(want)) or (np.isnan(sumsq_) and np.isnan(got[:2]).all() and (got[2:] == 0).all()), \
                (sumsq_, max_norm, scale, got, want)
            assert state.guards_intact()
            if np.isfinite(got[1]):
                assert got[3] == 1.0 and got[2] == np.float64(np.float32(got[2])) and 0.0 <= got[2] <= np.float64(np.float32(scale))
                if max_norm == float('inf'):
                    assert got[2] == np.float64(np.float32(scale)), 'max_norm = inf: the factor is float(grad_scale)'


def check_clip_finish_scaled_refusals(npm) -> None:
    _C, lib = _lib()
    start = np.array([4.0, -1.0, -1.0, -1.0])
    state = OC.Raw(npm, np.float64, 4, 0, start)
    for max_norm in (0.0, -1.0, float('nan')):
        assert lib.npm_clip_finish_scaled(state.ptr, max_norm, 0.5) == BAD_ARGUMENT, max_norm
    for scale in (0.0, -0.5, float('nan'), float('inf')):
        assert lib.npm_clip_finish_scaled(state.ptr, 1.0, scale) == BAD_ARGUMENT, scale
    assert lib.npm_clip_finish_scaled(None, 1.0, 0.5) == BAD_ARGUMENT
    assert np.array_equal(state.numpy(), start) and state.guards_intact()


# ---- the class and the trainer on a model -----------------------------------------------------------------------------------------------
LR, WEIGHT_DECAY = AC.LR, AC.WEIGHT_DECAY
K = 3                                                   # micro-batches of the fixture: one sequence each, 6 / 3 / 5 counted tokens


def holding(npm, *args, **kwargs):
    """An ``AdamWOptimizer`` that lists (obj, attribute) of every FIRST update of a step and, after every ``apply()``, keeps what the
    step was taken with: the gradients it held (the accumulators, folded) as host arrays."""
    class Holding(npm.optimizer.AdamWOptimizer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.seen, self.applies, self.used, self.lasts = [], 0, [], []

        def update(self, obj, attribute, gradient):
            if f'{id(obj)}.{attribute}' not in self._pending:
                self.seen.append((obj, attribute))
            super().update(obj, attribute, gradient)

        def apply(self, grad_scale=1.0):
            held = [g for _, _, g in self._pending.values()]
            self.applies += 1
            super().apply(grad_scale=grad_scale)
            self.used = [np.array(g, dtype=np.float32, copy=True) for g in held]
            self.lasts.append(self.last)

    return Holding(*args, **kwargs)


def train(npm, lm, optimizer, steps, micro_batches=1, loss_=None):
    _, inputs, targets = MC.tokens()
    loss_ = npm.loss.SoftmaxCrossEntropyLoss(reduction='sum') if loss_ is None else loss_
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        npm.train.Trainer([lm], loss_).train(inputs, targets, steps, optimizer, micro_batches=micro_batches)
    return out.getvalue()


def snapshot(opt):
    """(parameters, moments, clip state or None) as bit patterns."""
    items = opt.seen[:len(opt.seen) // max(opt.applies, 1)]
    params = [R.bits(p) for p in AC.parameters_of(items)]
    moments = [(R.bits(m), R.bits(v)) for m, v in AC.moments_of(opt, items)]
    state = R.bits(AC.clip_state(opt)) if opt._clip_state is not None else None
    return params, moments, state


def same_snapshot(a, b) -> bool:
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and len(a[0]) == len(b[0]) \
        and all(np.array_equal(m, n) and np.array_equal(v, w) for (m, v), (n, w) in zip(a[1], b[1])) \
        and ((a[2] is None and b[2] is None) or np.array_equal(a[2], b[2]))


def check_accumulate_with_one_backward_equals_plain(npm, steps=2) -> None:
    results = []
    for accumulate in (False, True):
        lm = MC.make_lm(npm)
        opt = holding(npm, LR, weight_decay=WEIGHT_DECAY, clip_norm=0.05, accumulate=accumulate)
        AC.train(npm, lm, opt, steps)
        assert opt.applies == steps and opt.last['folds'] == 0 and opt.last['fold_launches'] == 0 and not opt.last['fused_norm']
        results.append(snapshot(opt))
    assert len(results[0][0]) >= 20 and same_snapshot(*results), 'accumulate=True with one backward per apply() changes bits'


class Keeping(MC.Recorder):
    """``lm_cases.Recorder`` that also lists (owner, attribute) in update order."""

    def __init__(self):
        super().__init__()
        self.items = []

    def update(self, obj, attribute, gradient):
        super().update(obj, attribute, gradient)
        self.items.append((obj, attribute))


def micro_gradients(npm):
    """The K micro-gradients of the summed loss, as the device computes them, of an untouched model: ([per micro-batch: per
    parameter float32 arrays in update order], the model, the (owner, attribute) keys in that order)."""
    lm = MC.make_lm(npm)
    _, inputs, targets = MC.tokens()
    loss_ = npm.loss.SoftmaxCrossEntropyLoss(reduction='sum')
    out, keys, counts = [], None, []
    for j in range(K):
        loss_(lm(inputs[j:j + 1]), targets[j:j + 1])
        counts.append(loss_.count)
        rec = Keeping()
        lm(loss_(backprop=True), backprop=True, optimizer_=rec)
        assert keys is None or [(id(o), a) for o, a in keys] == list(rec.grads), 'the backward hands its gradients over in another order'
        keys = rec.items
        out.append([g.astype(np.float32) for g in rec.grads.values()])          # float64 copies of float32 gradients: exact
    assert counts == list(MC.LENGTHS) and len(set(counts)) > 1
    return out, lm, keys


def check_three_micro_batches(npm, fused=None, ranges=None) -> dict:
    """``Trainer.train(..., micro_batches=3)`` against the NumPy fold of the recorded micro-gradients, the clip model and the AdamW
    model.  ``fused`` / ``ranges`` set device.ACCUM_FUSED_NORM / device.ACCUM_RANGES for the run (None: as they are)."""
    from np_modeling_amd import device as D
    micro, untouched, keys = micro_gradients(npm)
    before = AC.parameters_of(keys)                     # an identical model that no optimizer has touched
    folded = [XR.fold([micro[j][i] for j in range(K)]) for i in range(len(micro[0]))]
    scale_ = 1.0 / sum(MC.LENGTHS)
    norm = scale_ * float(np.sqrt(AR.exact_sumsq(*folded)))
    assert np.isfinite(norm) and norm > 0
    clip_norm = 0.5 * norm

    trained = MC.make_lm(npm)
    saved = D.ACCUM_FUSED_NORM, D.ACCUM_RANGES
    try:
        D.ACCUM_FUSED_NORM = saved[0] if fused is None else fused
        D.ACCUM_RANGES = saved[1] if ranges is None else ranges
        use_ranges = D.ACCUM_RANGES is not False and hasattr(_lib()[1], 'npm_accumulate_ranges')       # (7 pairs: the ranges unless forced off)
        expect_fused = bool(D.ACCUM_FUSED_NORM and use_ranges)
        opt = holding(npm, LR, weight_decay=WEIGHT_DECAY, clip_norm=clip_norm, accumulate=True)
        printed = train(npm, trained, opt, 1, micro_batches=K)
    finally:
        D.ACCUM_FUSED_NORM, D.ACCUM_RANGES = saved
    assert opt.applies == 1 and printed.count('Step:') == 1 and printed.count('Loss:') == 1
    last = opt.last
    # adoption launches nothing: K micro-batches are K - 1 folds; every fold of this model is one call (one pair per bucket, < 32)
    assert last['folds'] == K - 1 and last['fused_norm'] == expect_fused, last
    assert last['fold_launches'] >= last['folds'] and last['updates'] == len(folded)
    for i, (got, want) in enumerate(zip(opt.used, folded)):
        assert np.array_equal(R.bits(got.ravel()), R.bits(want.ravel())), f'accumulator {i} is not the float32 fold in order'
    got_norm, factor, ok = opt.last_grad_norm()
    state = AC.clip_state(opt)
    out = {'norm error / bound': AR.sumsq_check(float(state[0]), folded, 'the device sum of squares'), 'scale': factor, 'ties': 0,
           'differing': 0, 'last': last}
    assert ok and factor == state[2] and got_norm == state[1] and factor < np.float32(scale_)
    assert np.array_equal(R.bits(state[1:]), R.bits(np.array(XR.clip_finish_scaled(state[0], clip_norm, scale_))))
    items = opt.seen
    assert [(type(o).__name__, a) for o, a in items] == [(type(o).__name__, a) for o, a in keys]
    for (obj, attribute), p0, g, (m1, v1) in zip(items, before, folded, AC.moments_of(opt, items)):
        wd = WEIGHT_DECAY if attribute.startswith('_w') else 0.0
        want = AR.adamw_model(p0.ravel(), g.ravel(), np.zeros(g.size), np.zeros(g.size), 1, (LR, 0.9, 0.999, 1e-8), wd, (factor, 1.0))
        got = np.array(getattr(obj, attribute), dtype=np.float32).ravel()
        exempt, differing = AR.adamw_check(got, m1, v1, want, what=f'{type(obj).__name__}.{attribute}')
        out['ties'] += exempt
        out['differing'] += differing
    out['snapshot'] = snapshot(opt)
    return out


def check_switches_agree(npm) -> dict:
    """Fused norm on and off, the ranges route and the axpy route: parameter, moment and clip-state bits."""
    runs = {(fused, ranges): check_three_micro_batches(npm, fused=fused, ranges=ranges) for fused in (True, False) for ranges in (True, False)}
    base = runs[(False, False)]['snapshot']
    for key, run in runs.items():
        assert same_snapshot(run['snapshot'], base), f'fused={key[0]} ranges={key[1]} changes bits'
    return {key: run['last'] for key, run in runs.items()}


def check_against_the_full_batch_in_float64(npm) -> float:
    """grad_scale x accumulator against ``lm_cases.reference_step``'s gradients of the mean loss of the whole batch; returns the
    worst error as a fraction of the bound (tests/accum_reference.py)."""
    from np_modeling_amd import _C
    _, scaled_bound = _C.parity_bounds()['f32']
    micro, lm, keys = micro_gradients(npm)
    _, inputs, targets = MC.tokens()
    _, _, full = MC.reference_step(lm, inputs, targets)
    refs = []
    for j in range(K):
        _, _, mean_grads = MC.reference_step(lm, inputs[j:j + 1], targets[j:j + 1])
        refs.append({key: MC.LENGTHS[j] * g for key, g in mean_grads.items()})       # the summed loss of micro-batch j
    scale_ = 1.0 / sum(MC.LENGTHS)
    worst = 0.0
    for i, (owner, attribute) in enumerate(keys):
        key = (id(owner), attribute)
        mine = [micro[j][i] for j in range(K)]
        theirs = [refs[j][key].reshape(mine[j].shape) for j in range(K)]
        for j in range(K):                                    # each micro-gradient meets the contract against its own counterpart
            assert np.abs(mine[j] - theirs[j]).max() <= XR.parity_bound(theirs[j], scaled_bound), (key[1], j)
        got = scale_ * XR.fold(mine).astype(np.float64)
        bound = XR.full_batch_bound(theirs, mine, scale_, scaled_bound)
        err = np.abs(got - full[key].reshape(got.shape))
        assert (err <= bound).all(), f'{key[1]}: {float((err / bound).max()):.3g} of the bound'
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


def check_second_update_folds_first_and_plain_still_raises(npm) -> None:
    class Holder:
        pass
    rng = np.random.default_rng(8)
    grads = [rng.standard_normal(37).astype(np.float32) for _ in range(3)]
    h = Holder()
    h._w = npm.device.zeros([37])
    opt = npm.optimizer.AdamWOptimizer(1e-3, clip_norm=1.0, accumulate=True)
    first = npm.device.from_host(grads[0])
    opt.update(h, '_w', first)
    assert opt._pending[f'{id(h)}._w'][2] is first and opt._folds == 0, 'the first gradient is adopted: nothing launched, nothing copied'
    opt.update(h, '_w', npm.device.from_host(grads[1]))
    assert opt._folds == 0 and len(opt._incoming) == 1
    opt.update(h, '_w', npm.device.from_host(grads[2]))       # the slot has an unfolded gradient: fold() runs first
    assert opt._folds == 1 and len(opt._incoming) == 1
    assert np.array_equal(R.bits(first.numpy()), R.bits(grads[0] + grads[1]))
    opt.fold()
    assert np.array_equal(R.bits(first.numpy()), R.bits(XR.fold(grads))) and not opt._incoming
    opt.fold()                                                # nothing to fold: nothing happens
    assert opt._folds == 2
    opt.apply(grad_scale=0.5)
    assert opt.last['folds'] == 2 and np.asarray(h._w).any()
    with np.testing.assert_raises(ValueError):
        opt.update(h, '_w', npm.device.zeros([36]))
    plain = npm.optimizer.AdamWOptimizer(1e-3)
    plain.update(h, '_w', npm.device.from_host(grads[0]))
    with np.testing.assert_raises(RuntimeError):
        plain.update(h, '_w', npm.device.from_host(grads[1]))


def check_thirty_three_pairs_through_the_optimizer(npm) -> dict:
    """33 parameters of their own buffers: every fold is two launches (32 + 1) on the ranges route, and the fused sum is split alike."""
    class Holder:
        pass
    rng = np.random.default_rng(3)
    holders = []
    grads = [[rng.standard_normal(5 + i).astype(np.float32) for i in range(33)] for _ in range(2)]
    for i in range(33):
        h = Holder()
        h._w = npm.device.zeros([5 + i])
        holders.append(h)
    opt = npm.optimizer.AdamWOptimizer(1e-3, clip_norm=1.0, accumulate=True)
    for micro in grads:
        for h, g in zip(holders, micro):
            opt.update(h, '_w', npm.device.from_host(g))
    opt.apply(grad_scale=0.5)
    folded = [a + b for a, b in zip(*grads)]
    AR.sumsq_check(float(AC.clip_state(opt)[0]), folded, '33 pairs')
    assert opt.last['ranges'] == 33 and opt.last['folds'] == 1
    return opt.last


def check_unclipped_scale(npm) -> None:
    """Without clip_norm a grad_scale still reaches the step (a zeroed state, max_norm = inf) and ``last_grad_norm`` keeps raising."""
    class Holder:
        pass
    rng = np.random.default_rng(12)
    p0, g = rng.standard_normal(257).astype(np.float32), rng.standard_normal(257).astype(np.float32)
    h = Holder()
    h._w = npm.device.from_host(p0)
    opt = npm.optimizer.AdamWOptimizer(LR, weight_decay=WEIGHT_DECAY, accumulate=True)
    opt.update(h, '_w', npm.device.from_host(g))
    opt.apply(grad_scale=1.0 / 3.0)
    want = AR.adamw_model(p0, g, np.zeros(257), np.zeros(257), 1, (LR, 0.9, 0.999, 1e-8), WEIGHT_DECAY, (np.float32(1.0 / 3.0), 1.0))
    (m1, v1), = AC.moments_of(opt, [(h, '_w')])
    AR.adamw_check(np.asarray(h._w), m1, v1, want, what='unclipped, scaled')
    with np.testing.assert_raises(RuntimeError):
        opt.last_grad_norm()


def check_trainer_refusals(npm) -> None:
    import pytest
    lm = MC.make_lm(npm)
    _, inputs, targets = MC.tokens()
    total = npm.loss.SoftmaxCrossEntropyLoss(reduction='sum')
    accumulating = npm.optimizer.AdamWOptimizer(1e-3, accumulate=True)
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match='divide'):
            npm.train.Trainer([lm], total).train(inputs, targets, 1, accumulating, micro_batches=2)           # B = 3
        with pytest.raises(ValueError, match='accumulat'):
            npm.train.Trainer([lm], total).train(inputs[:2], targets[:2], 1, npm.optimizer.SGDOptimizer(0.1), micro_batches=2)
        with pytest.raises(ValueError, match='accumulat'):
            npm.train.Trainer([lm], total).train(inputs[:2], targets[:2], 1, npm.optimizer.AdamWOptimizer(1e-3), micro_batches=2)
        with pytest.raises(ValueError, match='mean of per-micro-batch means'):
            npm.train.Trainer([lm], npm.loss.SoftmaxCrossEntropyLoss()).train(inputs[:2], targets[:2], 1, accumulating, micro_batches=2)
    assert not accumulating._pending


def check_printed_loss_is_the_token_mean(npm) -> None:
    """``Loss:`` with micro-batches and a summed loss is sum(loss_j) / sum(count_j): the mean loss of the whole batch."""
    lm = MC.make_lm(npm)
    _, inputs, targets = MC.tokens()
    mean = npm.loss.SoftmaxCrossEntropyLoss()
    want = float(mean(lm(inputs), targets, need_grad=False))
    opt = npm.optimizer.AdamWOptimizer(1e-3, accumulate=True)
    printed = train(npm, lm, opt, 1, micro_batches=K)
    got = float(printed.split('Loss:')[1].split()[0])
    from np_modeling_amd import _C
    print(f'printed {got!r}, the mean loss of one forward over the whole batch {want!r}')
    assert abs(got - want) <= _C.parity_bounds()['f32'][0] * abs(want), (got, want)        # the contract test_gpu_lm.py holds a loss to
