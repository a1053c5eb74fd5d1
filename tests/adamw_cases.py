"""TEST INFRASTRUCTURE: the cases and checks of npm_sumsq_ranges, npm_clip_finish, npm_adamw_step (csrc/npm_clip.hip) and of
``optimizer.AdamWOptimizer`` on a model, written once and run through whatever library ``np_modeling_amd._C`` holds: the host
simulator (tests/hostsim/) in tests/test_adamw_host.py, libnpm_hip.so in tests/test_gpu_adamw.py.  Models and bounds:
tests/adamw_reference.py.  Buffers with sentinel guards: tests/optim_cases.py ``F32`` / ``Raw``.

Sizes come from the launch code: a tile of the sum is 16384 elements (sizes around one tile, and three tiles and a bit: more than
one block, a short last tile); the step runs at most 4096 blocks of 256 threads, so 2^20 + 257 elements take a second trip of its
grid-stride loop."""

from __future__ import annotations

import contextlib
import ctypes as C
import io

import numpy as np

import adamw_reference as AR
import lm_cases as MC
import optim_cases as OC
import optim_reference as R

TILE = AR.TILE
BAD_ARGUMENT = OC.BAD_ARGUMENT
SUMSQ_SIZES = [0, 1, 3, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
SUMSQ_OFFSETS = [0, 1, 2, 3]            # floats in front of the range: every head and tail peel beside a 16-byte interior
SUMSQ_DATA = ['normal', 'huge', 'tiny', 'spike']


def _lib():
    from np_modeling_amd import _C
    return _C, _C.lib()


def sumsq_data(kind: str, n: int, rng) -> np.ndarray:
    """'normal': N(0, 1).  'huge': magnitudes 1e18 .. 3.2e19 -- above 1.85e19 the square itself overflows float32, and a float32
    sum of the others does after a few hundred.  'tiny': 1e-30 .. 2e-30, squares of 1e-60 that are zero in float32.  'spike':
    N(0, 1e-3) with one element of 1e6 in the middle."""
    if kind == 'normal':
        return rng.standard_normal(n).astype(np.float32)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    if kind == 'huge':
        return (sign * 1e18 * rng.uniform(1.0, 32.0, n)).astype(np.float32)
    if kind == 'tiny':
        return (sign * 1e-30 * rng.uniform(1.0, 2.0, n)).astype(np.float32)
    x = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    if n:
        x[n // 2] = 1e6
    return x


def ranges_table(parts):
    """npm_ranges from [(address or None, n), ...]."""
    from np_modeling_amd import _C
    table = _C.npm_ranges()
    for i, (ptr, n) in enumerate(parts):
        table.ptr[i], table.n[i] = ptr, n
    table.count = len(parts)
    return table


def sumsq(npm, parts, acc) -> float:
    _C, lib = _lib()
    table = ranges_table(parts)
    _C.check(lib.npm_sumsq_ranges(C.byref(table), acc.ptr), 'npm_sumsq_ranges')
    return float(acc.numpy()[0])


def check_sumsq_single(npm, kind: str) -> float:
    """One range of every size at every offset; returns the worst error as a fraction of the bound."""
    worst = 0.0
    for n in SUMSQ_SIZES:
        for offset in SUMSQ_OFFSETS:
            rng = np.random.default_rng(1000 * n + offset)
            x = sumsq_data(kind, n, rng)
            buf = OC.F32(npm, n, offset, x if n else None)
            acc = OC.Raw(npm, np.float64, 1, 8, np.zeros(1))
            got = sumsq(npm, [(buf.ptr, n)], acc)
            what = f'{kind} n={n} offset={offset}'
            worst = max(worst, AR.sumsq_check(got, [x], what))
            again = OC.Raw(npm, np.float64, 1, 8, np.zeros(1))
            assert R.bits(np.float64(sumsq(npm, [(buf.ptr, n)], again))) == R.bits(np.float64(got)), f'{what}: a repeated call differs'
            assert acc.guards_intact() and buf.guards_intact(), f'{what}: a guard was written'
            assert np.array_equal(R.bits(buf.numpy()), R.bits(x)), f'{what}: the input was written'
    return worst


def check_sumsq_tables(npm) -> dict:
    """Several ranges in one call: zero-length ranges in the middle (one with a NULL address), one range cut into two adjacent
    ones, 32 ranges; two calls accumulate.  Returns error / bound per check."""
    rng = np.random.default_rng(77)
    sizes = [TILE + 3, 0, 5, 0, 2 * TILE, 257]
    data = [sumsq_data('normal', n, rng) for n in sizes]
    bufs = [OC.F32(npm, n, i % 4, x if n else None) for i, (n, x) in enumerate(zip(sizes, data))]
    parts = [(b.ptr, n) for b, n in zip(bufs, sizes)]
    parts[3] = (None, 0)
    out = {}
    acc = OC.Raw(npm, np.float64, 1, 0, np.zeros(1))
    out['zero-length in the middle'] = AR.sumsq_check(sumsq(npm, parts, acc), data, 'zero-length ranges')
    # accumulation: the same table again, onto what is there
    first = float(acc.numpy()[0])
    second = sumsq(npm, parts, acc)
    fresh = OC.Raw(npm, np.float64, 1, 0, np.zeros(1))
    assert R.bits(np.float64(sumsq(npm, parts, fresh))) == R.bits(np.float64(first))
    assert second == first + first, 'two calls do not accumulate'
    out['two calls'] = AR.sumsq_check(second, data + data, 'two calls')
    # one range against the same memory as two adjacent ranges, cut inside a tile and off a 16-byte boundary
    n = 3 * TILE + 5
    x = sumsq_data('spike', n, rng)
    whole = OC.F32(npm, n, 1, x)
    one, two = (OC.Raw(npm, np.float64, 1, 0, np.zeros(1)) for _ in range(2))
    cut = TILE + 1001
    out['one range'] = AR.sumsq_check(sumsq(npm, [(whole.ptr, n)], one), [x], 'one range')
    out['cut in two'] = AR.sumsq_check(sumsq(npm, [(whole.ptr, cut), (whole.ptr + 4 * cut, n - cut)], two), [x], 'cut in two')
    # a full table
    sizes = [1 + 37 * i for i in range(32)]
    data = [sumsq_data('normal', k, rng) for k in sizes]
    bufs32 = [OC.F32(npm, k, i % 4, d) for i, (k, d) in enumerate(zip(sizes, data))]
    full = OC.Raw(npm, np.float64, 1, 0, np.zeros(1))
    out['32 ranges'] = AR.sumsq_check(sumsq(npm, [(b.ptr, k) for b, k in zip(bufs32, sizes)], full), data, '32 ranges')
    for b in bufs + bufs32 + [whole, acc, one, two, full]:
        assert b.guards_intact(), 'a guard was written'
    return out


def check_sumsq_arguments(npm) -> None:
    _C, lib = _lib()
    acc = OC.Raw(npm, np.float64, 1, 0, np.zeros(1))
    buf = OC.F32(npm, 8, 0, np.ones(8, dtype=np.float32))
    for parts in ([], [(buf.ptr, 0)], [(None, 0), (buf.ptr, 0)]):
        table = ranges_table(parts)
        assert lib.npm_sumsq_ranges(C.byref(table), acc.ptr) == 0
    assert float(acc.numpy()[0]) == 0.0
    bad = ranges_table([(None, 3)])
    assert lib.npm_sumsq_ranges(C.byref(bad), acc.ptr) == BAD_ARGUMENT
    for count in (-1, 33):
        table = ranges_table([(buf.ptr, 8)])
        table.count = count
        assert lib.npm_sumsq_ranges(C.byref(table), acc.ptr) == BAD_ARGUMENT
    ok = ranges_table([(buf.ptr, 8)])
    assert lib.npm_sumsq_ranges(C.byref(ok), None) == BAD_ARGUMENT
    assert float(acc.numpy()[0]) == 0.0 and acc.guards_intact()


# ---- the clip factor ------------------------------------------------------------------------------------------------------------------
# (sumsq, max_norm)
CLIP_CASES = [(4.0, 3.0), (4.0, 2.0), (4.0, 1.0), (1e6, 1.0), (123.456, 0.37), (2.0, float('inf')), (0.0, 1.0), (1e-20, 1.0),
              (float('inf'), 1.0), (float('nan'), 1.0), (1e300, 1e-3)]


def check_clip_finish(npm) -> None:
    _C, lib = _lib()
    for sumsq_, max_norm in CLIP_CASES:
        state = OC.Raw(npm, np.float64, 4, 8, np.array([sumsq_, -1.0, -1.0, -1.0]))
        _C.check(lib.npm_clip_finish(state.ptr, max_norm), 'npm_clip_finish')
        got = state.numpy()
        want = np.array([sumsq_, *AR.clip_finish(sumsq_, max_norm)])
        assert np.array_equal(R.bits(got), R.bits(want)) or (np.isnan(sumsq_) and np.isnan(got[:2]).all() and (got[2:] == 0).all()), \
            (sumsq_, max_norm, got, want)
        assert state.guards_intact()
        norm = np.sqrt(np.float64(sumsq_))
        if not np.isfinite(norm):
            assert got[2] == 0.0 and got[3] == 0.0
        else:
            assert got[3] == 1.0 and got[2] == np.float64(np.float32(got[2]))         # exactly a float
            if norm + 1e-6 <= max_norm:
                assert got[2] == 1.0
            else:
                assert got[2] < 1.0
    state = OC.Raw(npm, np.float64, 4, 0, np.array([4.0, -1.0, -1.0, -1.0]))
    for bad in (0.0, -1.0, float('nan')):
        assert lib.npm_clip_finish(state.ptr, bad) == BAD_ARGUMENT
    assert lib.npm_clip_finish(None, 1.0) == BAD_ARGUMENT
    assert np.array_equal(state.numpy(), [4.0, -1.0, -1.0, -1.0])


# ---- the step -------------------------------------------------------------------------------------------------------------------------
STEP_SIZES = [1, 257, OC.EW_SEAM + 257]
STEP_DECAYS = [0.0, 0.1]
STEP_CLIPS = ['null', 'one', 'scaled', 'skip']
STEP_CASES = [(n, wd, clip) for n in STEP_SIZES for wd in STEP_DECAYS for clip in STEP_CLIPS]
STEP_SEED = 40
_CLIP_STATE = {'one': (9.0, 3.0, 1.0, 1.0), 'scaled': (65.7, 8.1, float(np.float32(0.37)), 1.0), 'skip': (float('inf'), float('inf'), 0.0, 0.0)}


def step_case_id(case) -> str:
    return f'n{case[0]}-wd{case[1]:g}-{case[2]}'


def check_step_case(npm, case, stepper=None) -> list:
    """Three steps from zero moments, the parameter at float offset 1, the gradient at 3, the moments one double in; each step's
    model starts from the state read back after the step before.  ``stepper(p, g, m, v, step, wd, clip) -> (p, m, v)`` replaces
    the library.  Returns [(step, near ties, near ties where the parameter differs)]."""
    n, wd, kind = case
    rng = np.random.default_rng(STEP_SEED + n)
    p0 = rng.standard_normal(n).astype(np.float32)
    p, m, v = p0, np.zeros(n), np.zeros(n)
    state = _CLIP_STATE.get(kind)
    clip = None if state is None else (state[2], state[3])
    if stepper is None:
        _C, lib = _lib()
        dp = OC.F32(npm, n, 1, p0)
        dm, dv = (OC.Raw(npm, np.float64, n, 8, np.zeros(n)) for _ in range(2))
        dstate = None if state is None else OC.Raw(npm, np.float64, 4, 8, np.array(state))
        if kind == 'one':                                           # the same steps with clip_state = NULL beside it
            twin = OC.F32(npm, n, 1, p0), OC.Raw(npm, np.float64, n, 8, np.zeros(n)), OC.Raw(npm, np.float64, n, 8, np.zeros(n))
    used = []
    for step in (1, 2, 3):
        g = R.adam_gradient(rng, n)
        want = AR.adamw_model(p, g, m, v, step, AR.HYPER, wd, clip)
        if stepper is None:
            dg = OC.F32(npm, n, 3, g)
            _C.check(lib.npm_adamw_step(dp.ptr, dg.ptr, dm.ptr, dv.ptr, n, *AR.HYPER, step, wd, dstate.ptr if dstate else None),
                     'npm_adamw_step')
            got = dp.numpy(), dm.numpy(), dv.numpy()
            assert dp.guards_intact() and dm.guards_intact() and dv.guards_intact() and dg.guards_intact(), 'a guard was written'
            assert np.array_equal(R.bits(dg.numpy()), R.bits(g)), 'the gradient was written'
            if dstate is not None:
                assert dstate.guards_intact() and np.array_equal(R.bits(dstate.numpy()), R.bits(np.array(state))), 'the clip state was written'
            if kind == 'one':
                _C.check(lib.npm_adamw_step(twin[0].ptr, dg.ptr, twin[1].ptr, twin[2].ptr, n, *AR.HYPER, step, wd, None), 'npm_adamw_step')
                for a, b in zip(got, twin):
                    assert np.array_equal(R.bits(a), R.bits(b.numpy())), 'scale 1 does not give the bits of clip_state = NULL'
        else:
            got = stepper(p, g, m, v, step, wd, clip)
        what = f'{step_case_id(case)} step {step}'
        exempt, differing = AR.adamw_check(*got, want, what=what)
        if kind == 'skip':
            assert np.array_equal(R.bits(got[0]), R.bits(p)) and np.array_equal(R.bits(got[1]), R.bits(m)) \
                and np.array_equal(R.bits(got[2]), R.bits(v)), f'{what}: ok = 0 changed something'
        elif step == 1 and wd == 0:
            zero = g == 0
            assert np.array_equal(R.bits(got[0][zero]), R.bits(p[zero])), 'g == 0 at step 1 without decay changed the parameter'
        used.append((step, exempt, differing))
        p, m, v = got
    return used


def check_step_arguments(npm) -> None:
    _C, lib = _lib()
    p, g = OC.F32(npm, 8, 0, np.ones(8, dtype=np.float32)), OC.F32(npm, 8, 0, np.ones(8, dtype=np.float32))
    m, v = (OC.Raw(npm, np.float64, 8, 0, np.zeros(8)) for _ in range(2))
    args = [p.ptr, g.ptr, m.ptr, v.ptr, 8, *AR.HYPER, 1, 0.1, None]
    for index, value in ((9, 0), (10, -0.5), (0, None), (1, None), (2, None), (3, None)):
        bad = list(args)
        bad[index] = value
        assert lib.npm_adamw_step(*bad) == BAD_ARGUMENT, (index, value)
    empty = list(args)
    empty[4] = 0
    empty[0] = None
    assert lib.npm_adamw_step(*empty) == 0
    assert np.array_equal(p.numpy(), np.ones(8)) and not m.numpy().any() and not v.numpy().any()
    assert all(b.guards_intact() for b in (p, g, m, v))


# ---- the class on a model -------------------------------------------------------------------------------------------------------------
class Recorder:
    """An optimizer that copies every gradient to the host, in the order the backward hands them over, and updates nothing."""

    def __init__(self):
        self.items = []                                 # (obj, attribute, float32 gradient)

    def update(self, obj, attribute, gradient):
        self.items.append((obj, attribute, np.array(gradient, dtype=np.float32, copy=True)))


def watching(npm, *args, **kwargs):
    """An ``AdamWOptimizer`` that also lists (obj, attribute) of every ``update``."""
    class Watching(npm.optimizer.AdamWOptimizer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.seen, self.applies = [], 0

        def update(self, obj, attribute, gradient):
            self.seen.append((obj, attribute))
            super().update(obj, attribute, gradient)

        def apply(self):
            self.applies += 1
            super().apply()

    return Watching(*args, **kwargs)


def clip_state(optimizer) -> np.ndarray:
    """[sumsq, norm, scale, ok] of the optimizer's most recent clipped apply()."""
    from np_modeling_amd import _C
    state = np.zeros(4)
    _C.check(_C.lib().npm_d2h(state.ctypes.data, optimizer._clip_state.ptr, 32), 'npm_d2h')
    return state


def moments_of(optimizer, items) -> list:
    """[(first, second)] moments of every (obj, attribute), read back from the optimizer's device buffers."""
    out = []
    for obj, attribute, *_ in items:
        state, n = optimizer._state[f'{id(obj)}.{attribute}'][1], getattr(obj, attribute).size
        out.append((_doubles(state.first_ptr, n), _doubles(state.second_ptr, n)))
    return out


def parameters_of(items) -> list:
    return [np.array(getattr(obj, attribute), dtype=np.float32, copy=True) for obj, attribute, *_ in items]


def train(npm, lm, optimizer, steps, loss_=None):
    _, inputs, targets = MC.tokens()
    loss_ = npm.loss.SoftmaxCrossEntropyLoss() if loss_ is None else loss_
    with contextlib.redirect_stdout(io.StringIO()):
        npm.train.Trainer([lm], loss_).train(inputs, targets, steps, optimizer)


LR, WEIGHT_DECAY = 1e-2, 0.1


def check_class_on_model(npm) -> dict:
    """Two identical models: one backward with a ``Recorder``, one ``Trainer`` step with ``AdamWOptimizer(clip_norm=c)``, c half
    the recorded norm.  The device norm against the fp64 norm of the recorded gradients; every parameter against the model of the
    step applied to the recorded gradients with the device's factor."""
    recorded, trained = MC.make_lm(npm), MC.make_lm(npm)
    _, inputs, targets = MC.tokens()
    loss_ = npm.loss.SoftmaxCrossEntropyLoss()
    loss_(recorded(inputs), targets)
    rec = Recorder()
    recorded(loss_(backprop=True), backprop=True, optimizer_=rec)
    grads = [g for _, _, g in rec.items]
    norm = float(np.sqrt(AR.exact_sumsq(*grads)))
    assert np.isfinite(norm) and norm > 0
    before = parameters_of(rec.items)

    opt = watching(npm, LR, weight_decay=WEIGHT_DECAY, clip_norm=0.5 * norm)
    train(npm, trained, opt, 1)
    assert [(type(o).__name__, a) for o, a in opt.seen] == [(type(o).__name__, a) for o, a, _ in rec.items] and opt.applies == 1
    got_norm, scale, ok = opt.last_grad_norm()
    state = clip_state(opt)
    assert ok and scale < 1.0 and scale == state[2] and got_norm == state[1]
    out = {'norm error / bound': AR.sumsq_check(float(state[0]), grads, 'the device norm'), 'scale': scale, 'ties': 0, 'differing': 0}
    assert np.array_equal(R.bits(state[1:]), R.bits(np.array(AR.clip_finish(state[0], 0.5 * norm))))
    for (obj, attribute), p0, g, (first, second) in zip(opt.seen, before, grads, moments_of(opt, opt.seen)):
        wd = WEIGHT_DECAY if attribute.startswith('_w') else 0.0
        want = AR.adamw_model(p0.ravel(), g.ravel(), np.zeros(g.size), np.zeros(g.size), 1, (LR, 0.9, 0.999, 1e-8), wd, (scale, 1.0))
        got = np.array(getattr(obj, attribute), dtype=np.float32).ravel()
        exempt, differing = AR.adamw_check(got, first, second, want, what=f'{type(obj).__name__}.{attribute}')
        out['ties'] += exempt
        out['differing'] += differing
    assert opt.last['updates'] == len(grads)
    return out


def check_coalesced_equals_per_parameter(npm, steps=3) -> None:
    from np_modeling_amd import device as D
    results = []
    saved = D.COALESCE_UPDATES
    try:
        for flag in (True, False):
            D.COALESCE_UPDATES = flag
            lm = MC.make_lm(npm)
            opt = watching(npm, LR, weight_decay=WEIGHT_DECAY, clip_norm=0.05)
            train(npm, lm, opt, steps)
            assert opt.applies == steps and opt.last_grad_norm()[1] < 1.0
            count = len(opt.seen) // steps
            results.append((parameters_of(opt.seen[:count]), opt.last))
    finally:
        D.COALESCE_UPDATES = saved
    (joined, last_joined), (single, last_single) = results
    assert len(joined) == len(single) and len(joined) >= 20
    for a, b in zip(joined, single):
        assert np.array_equal(R.bits(a), R.bits(b))
    assert last_single['launches'] == last_single['updates'] and last_joined['launches'] < last_joined['updates']


class InfLoss:
    """``SoftmaxCrossEntropyLoss`` whose gradient holds one +inf."""

    def __init__(self, npm):
        self._inner = npm.loss.SoftmaxCrossEntropyLoss()

    def resident_targets(self, targets):
        return self._inner.resident_targets(targets)

    def __call__(self, *args, backprop=False, **kwargs):
        out = self._inner(*args, backprop=backprop, **kwargs)
        if backprop:
            host = np.array(out, dtype=np.float32)
            host.reshape(-1)[7] = np.inf
            out.set(host)
        return out


def check_non_finite_step_is_skipped(npm) -> None:
    lm = MC.make_lm(npm)
    opt = watching(npm, LR, weight_decay=WEIGHT_DECAY, clip_norm=1.0)
    train(npm, lm, opt, 1)                               # a sound step first: the moments are no longer zero
    items = list(opt.seen)
    before = parameters_of(items)
    m_before = moments_of(opt, items)
    train(npm, lm, opt, 1, InfLoss(npm))
    norm, scale, ok = opt.last_grad_norm()
    assert not ok and scale == 0.0 and not np.isfinite(norm)
    for a, b in zip(before, parameters_of(items)):
        assert np.array_equal(R.bits(a), R.bits(b)), 'a skipped step changed a parameter'
    for (m0, v0), (m1, v1) in zip(m_before, moments_of(opt, items)):
        assert np.array_equal(R.bits(m0), R.bits(m1)) and np.array_equal(R.bits(v0), R.bits(v1)), 'a skipped step changed a moment'
    assert any(np.abs(m0).max() > 0 for m0, _ in m_before)


def _doubles(ptr, n) -> np.ndarray:
    from np_modeling_amd import _C
    out = np.zeros(int(n))
    if n:
        _C.check(_C.lib().npm_d2h(out.ctypes.data, ptr, 8 * int(n)), 'npm_d2h')
    return out
