"""CPU: AdamW, global-norm clipping and the learning-rate schedule without a GPU, on the host simulator (tests/hostsim/; the three
entry points join it with the profile 'adamw').

* the cases of tests/adamw_cases.py, so that every check of tests/test_gpu_adamw.py has run (and the near-tie count of every step
  case has been asserted from the model alone) before a GPU sees it;
* the checks themselves: a float32 accumulator and a float32 square each miss the sum's bound by orders of magnitude, and three
  wrong models of the step (Adam's epsilon inside the root, Adam's float32 gradient products, a coupled decay) each fail;
* the host logic of ``optimizer.AdamWOptimizer``: nothing moves before ``apply()``, the call order of a step, no copy to the host,
  launches and ranges per arena, padding that never enters the norm, the schedule, ``Trainer`` calling ``apply()`` once a step and
  leaving ``SGDOptimizer``'s calls as they were (tests/golden/trainer_sgd_calls.json, recorded before ``Trainer`` looked for it)."""

import json
import math
import os

import numpy as np
import pytest

import adamw_cases as AC
import adamw_reference as AR
import lm_cases as MC
import optim_cases as OC
import optim_reference as R
from hostsim.fixtures import built, npm_fixture  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

npm = npm_fixture()


# ---- the same cases as on the GPU -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', AC.SUMSQ_DATA)
def test_sumsq_one_range(npm, kind):
    print('worst error / bound:', AC.check_sumsq_single(npm, kind))


def test_sumsq_tables_and_arguments(npm):
    print('error / bound:', AC.check_sumsq_tables(npm))
    AC.check_sumsq_arguments(npm)


def test_clip_finish(npm):
    AC.check_clip_finish(npm)


@pytest.mark.parametrize('case', AC.STEP_CASES, ids=AC.step_case_id)
def test_step_cases_and_their_near_tie_counts(npm, case):
    """The model alone first: the cap of 16 near ties a case holds before any library runs it."""
    alone = AC.check_step_case(None, case, stepper=lambda p, g, m, v, step, wd, clip: AR.adamw_model(p, g, m, v, step, AR.HYPER, wd, clip)[:3])
    assert all(exempt <= AR.MAX_EXEMPT for _, exempt, _ in alone)
    if case[0] > 4096 and (case[1], case[2]) != (0.1, 'scaled'):
        return                                           # the simulator IS the model: one large case through it is enough
    used = AC.check_step_case(npm, case)
    print('near ties (step, in the case, differing):', used)
    assert used == alone and all(differing == 0 for _, _, differing in used)


def test_step_arguments(npm):
    AC.check_step_arguments(npm)


def test_class_on_a_model(npm):
    out = AC.check_class_on_model(npm)
    print(out)
    assert out['differing'] == 0


def test_coalesced_equals_per_parameter(npm):
    AC.check_coalesced_equals_per_parameter(npm)


def test_a_non_finite_norm_skips_the_step(npm):
    AC.check_non_finite_step_is_skipped(npm)


# ---- the checks catch what they are there for -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['huge', 'tiny', 'spike', 'normal'])
def test_float32_sums_miss_the_bound_by_orders_of_magnitude(kind):
    n = 3 * AC.TILE + 5
    x = AC.sumsq_data(kind, n, np.random.default_rng(5))
    exact, bound = AR.exact_sumsq(x), AR.sumsq_bound(n, AR.exact_sumsq(x))
    with np.errstate(all='ignore'):
        f32_square = float((x * x).astype(np.float64).sum())                       # the square rounded to float32, summed in fp64
        f32_acc = float(np.cumsum((x.astype(np.float64) ** 2).astype(np.float32), dtype=np.float32)[-1])    # a float32 running sum
    for name, got in (('float32 square', f32_square), ('float32 accumulator', f32_acc)):
        err = abs(got - exact)
        print(f'{kind}: {name}: error / bound = {err / bound:.3g}')
        # N(0, 1): the float32 squares' rounding errors are random and partly cancel -- still tens of times the bound
        assert not err <= (10 if kind == 'normal' else 100) * bound, (kind, name)
        with pytest.raises(AssertionError):
            AR.sumsq_check(got, [x], name)
    assert AR.sumsq_check(float(np.sum(x.astype(np.float64) ** 2)), [x]) <= 1.0     # NumPy's pairwise fp64 sum is inside


@pytest.mark.parametrize('variant', ['eps_inside', 'f32_products', 'coupled'])
def test_wrong_models_of_the_step_fail(variant):
    case = (4099, 0.1, 'scaled')
    with pytest.raises(AssertionError):
        AC.check_step_case(None, case, stepper=lambda p, g, m, v, step, wd, clip: AR.adamw_model(p, g, m, v, step, AR.HYPER, wd, clip,
                                                                                                  variant=variant)[:3])


def test_model_against_torch_adamw_in_float64():
    """One step of ``torch.optim.AdamW`` in float64 on the CPU from the same float32 state; half a float32 ulp of the parameter
    (the model rounds once) plus 1e-12 |p| (torch orders its fp64 operations differently).  The kernel is held to the model."""
    torch = pytest.importorskip('torch')
    rng = np.random.default_rng(9)
    n = 4099
    p0, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    lr, b1, b2, eps = AR.HYPER
    for wd in (0.0, 0.1):
        want = AR.adamw_model(p0, g, np.zeros(n), np.zeros(n), 1, AR.HYPER, wd, None)
        t = torch.tensor(p0.astype(np.float64), requires_grad=True)
        opt = torch.optim.AdamW([t], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        t.grad = torch.tensor(g.astype(np.float64))
        opt.step()
        theirs = t.detach().numpy()
        half_ulp = np.spacing(np.abs(want.p)).astype(np.float64) / 2
        assert (np.abs(want.p.astype(np.float64) - theirs) <= half_ulp + 1e-12 * np.abs(theirs)).all()


# ---- the class ------------------------------------------------------------------------------------------------------------------------
def _backward(npm, lm, opt):
    _, inputs, targets = MC.tokens()
    loss_ = npm.loss.SoftmaxCrossEntropyLoss()
    loss_(lm(inputs), targets)
    lm(loss_(backprop=True), backprop=True, optimizer_=opt)


def test_update_changes_nothing_until_apply_and_aliases_see_the_step(npm):
    lm = MC.make_lm(npm)
    opt = AC.watching(npm, 1e-2, clip_norm=1.0)
    alias = lm.head._w
    _backward(npm, lm, opt)
    before = AC.parameters_of(opt.seen)
    assert 'npm_adamw_step' not in npm.sim.calls and opt.last is None
    with pytest.raises(RuntimeError, match=r'apply\(\)'):
        opt.update(*opt.seen[0], npm.device.zeros(getattr(*opt.seen[0]).shape))
    for a, b in zip(before, AC.parameters_of(opt.seen)):
        assert np.array_equal(R.bits(a), R.bits(b))
    head_before = np.array(alias, copy=True)
    opt.apply()
    assert lm.head._w is alias and not np.array_equal(np.asarray(alias), head_before)
    assert all(not np.array_equal(a, b) for a, b in zip(before, AC.parameters_of(opt.seen)) if a.size)
    calls = len(npm.sim.calls)
    opt.apply()                                          # nothing pending: nothing happens
    assert len(npm.sim.calls) == calls


def test_host_operands_are_refused(npm):
    class Holder:
        pass
    holder, opt = Holder(), npm.optimizer.AdamWOptimizer(1e-3)
    holder._w = np.ones(4, dtype=np.float32)
    with pytest.raises(TypeError, match='device-only'):
        opt.update(holder, '_w', np.ones(4, dtype=np.float32))
    holder._w = npm.device.zeros([4])
    with pytest.raises(TypeError, match='device-only'):
        opt.update(holder, '_w', np.ones(4, dtype=np.float32))
    opt.update(holder, '_w', 2.0 * npm.device.full([4], 1.0))           # a device.Scaled gradient is materialised
    opt.apply()
    assert np.asarray(holder._w)[0] < 0
    with pytest.raises(ValueError):
        npm.optimizer.AdamWOptimizer(1e-3, weight_decay=-0.1)
    with pytest.raises(ValueError):
        npm.optimizer.AdamWOptimizer(1e-3, clip_norm=0.0)
    with pytest.raises(RuntimeError):
        opt.last_grad_norm()                             # that apply() did not clip


def _with_fills(sim, start, fills):
    """``calls[start:]`` with an 'npm_fill_f64' back at every place where the runtime noted one in ``fills64[fills:]``: it keeps
    them out of ``calls``, as (len(calls) at the time, n)."""
    calls = sim.calls[start:]
    for at, _ in reversed(sim.fills64[fills:]):            # from the last: an insertion moves only what follows it
        calls.insert(at - start, 'npm_fill_f64')
    return calls


def test_the_calls_of_a_step_and_no_copy_to_the_host(npm):
    lm = MC.make_lm(npm)
    opt = AC.watching(npm, 1e-2, clip_norm=1.0)
    for step in range(3):
        _backward(npm, lm, opt)
        start, d2h, fills = len(npm.sim.calls), len(npm.sim.d2h), len(npm.sim.fills64)
        opt.apply()
        calls = _with_fills(npm.sim, start, fills)
        assert len(npm.sim.d2h) == d2h, 'apply() copied to the host'
        sums = math.ceil(opt.last['ranges'] / 32)
        if step:                                         # the first apply() also zeroes the moment buffers it creates
            assert calls[:1 + sums + 1] == ['npm_fill_f64'] + ['npm_sumsq_ranges'] * sums + ['npm_clip_finish']
            assert set(calls[2 + sums:]) == {'npm_adamw_step'} and len(calls) == 2 + sums + opt.last['launches']
        else:
            assert calls[:1 + sums + 1] == ['npm_fill_f64'] + ['npm_sumsq_ranges'] * sums + ['npm_clip_finish']
            assert set(calls[2 + sums:]) == {'npm_adamw_step', 'npm_fill_f64'}
        assert opt.last['updates'] == len(opt.seen) // (step + 1)
    d2h = len(npm.sim.d2h)
    opt.last_grad_norm()
    assert npm.sim.d2h[d2h:] == [32]


def test_thirty_three_ranges_take_two_launches_of_the_sum(npm):
    class Holder:
        pass
    rng = np.random.default_rng(3)
    holders, grads = [], []
    for i in range(33):
        h = Holder()
        h._w = npm.device.zeros([5 + i])
        holders.append(h)
        grads.append(rng.standard_normal(5 + i).astype(np.float32))
    opt = npm.optimizer.AdamWOptimizer(1e-3, clip_norm=1.0)
    for h, g in zip(holders, grads):
        opt.update(h, '_w', npm.device.from_host(g))
    start = len(npm.sim.calls)
    opt.apply()
    assert opt.last['ranges'] == 33 and npm.sim.calls[start:].count('npm_sumsq_ranges') == 2
    assert [len(t) for t in npm.sim.sumsq_tables[-2:]] == [32, 1]
    AR.sumsq_check(float(AC.clip_state(opt)[0]), grads, '33 ranges')


def _arena_runs(lm, opt, decays):
    """Maximal runs of equal decay among neighbours of each arena, from the parameters' own addresses."""
    items = sorted(((getattr(o, a)._buf.ptr, getattr(o, a).ptr, getattr(o, a).size, decays(o, a)) for o, a in opt.seen))
    runs, last = 0, None
    for buf, ptr, n, decay in items:
        if last is None or last[0] != buf or not 0 <= ptr - last[1] <= 12 or last[2] != decay:
            runs += 1
        last = (buf, ptr + 4 * n, decay)
    return runs, len({buf for buf, *_ in items})


def test_launches_per_arena_follow_the_decay(npm):
    for decay, same in ((None, False), (lambda *_: True, True), (lambda *_: False, True)):
        lm = MC.make_lm(npm)
        opt = AC.watching(npm, 1e-2, clip_norm=1.0, decay=decay)
        _backward(npm, lm, opt)
        opt.apply()
        runs, arenas = _arena_runs(lm, opt, opt.decay)
        print('decay', decay, 'launches', opt.last['launches'], 'arenas', arenas, 'updates', opt.last['updates'])
        assert opt.last['launches'] == runs
        if same:
            assert runs == arenas                        # one launch per arena
        else:
            assert runs > arenas


def test_one_range_per_arena_whose_segments_are_multiples_of_four_and_padding_never_enters_the_norm(npm):
    """F = 32 and hidden = 48: every matrix and vector of a block is a multiple of 4 floats, so a block's gradients are gap-free
    in its bucket.  Then a layer with odd sizes, its bucket poisoned: the simulator's fresh memory is NaN wherever nothing was
    written, the alignment padding between the slices included."""
    lm = MC.make_lm(npm)
    opt = AC.watching(npm, 1e-2, clip_norm=1.0)
    _backward(npm, lm, opt)
    grads_of = [g for _, _, g in opt._pending.values()]
    opt.apply()
    sizes = {}
    for o, a in opt.seen:
        sizes.setdefault(getattr(o, a)._buf.ptr, []).append(getattr(o, a).size)
    whole = [buf for buf, each in sizes.items() if all(n % 4 == 0 for n in each)]
    assert len(sizes) == 3 + MC.LAYERS and len(whole) == len(sizes) - 1       # the head's bias has VOCAB = 50 elements: a gap of 2
    assert opt.last['ranges'] == len(whole) + 2
    assert [len(t) for t in npm.sim.sumsq_tables[-1:]] == [opt.last['ranges']]
    per_buffer = {}
    for ptr, n in npm.sim.sumsq_tables[-1]:
        owner = [g._buf.ptr for g in grads_of if g.ptr <= ptr < g.ptr + 4 * g.size]
        per_buffer[owner[0]] = per_buffer.get(owner[0], 0) + 1
    assert sorted(per_buffer.values()) == [1] * len(whole) + [2]
    assert opt.last_grad_norm()[2]

    np.random.seed(4)
    dense = npm.layers.Linear(units=7)
    x = np.random.standard_normal([5, 3]).astype(np.float32)
    dense(x)
    odd = AC.watching(npm, 1e-2, clip_norm=1.0)
    dense(np.random.standard_normal([5, 7]).astype(np.float32), backprop=True, optimizer_=odd)
    sizes = [getattr(o, a).size for o, a in odd.seen]
    assert any(n % 4 for n in sizes[:-1]), sizes
    grads = [np.array(g, dtype=np.float32) for _, _, g in odd._pending.values()]
    odd.apply()
    norm, scale, ok = odd.last_grad_norm()
    assert ok and np.isfinite(norm) and odd.last['ranges'] >= 2
    AR.sumsq_check(float(AC.clip_state(odd)[0]), grads, 'odd sizes')


def test_a_callable_learning_rate_is_called_once_per_apply(npm):
    seen = []

    def rate(step):
        seen.append(step)
        return 1e-3

    lm = MC.make_lm(npm)
    opt = AC.watching(npm, rate)
    AC.train(npm, lm, opt, 3)
    assert seen == [1, 2, 3] and opt.applies == 3


def test_warmup_cosine_at_its_defining_points(npm):
    rate = npm.optimizer.warmup_cosine(2e-3, 10, 110, floor=2e-4)
    assert rate(1) == 2e-3 / 10 and rate(10) == 2e-3
    assert rate(60) == pytest.approx((2e-3 + 2e-4) / 2, rel=1e-12)
    assert rate(110) == 2e-4 and rate(500) == 2e-4
    assert all(rate(s) < rate(s + 1) for s in range(1, 10)) and all(rate(s) > rate(s + 1) for s in range(10, 110))
    assert npm.optimizer.warmup_cosine(1.0, 0, 4)(4) == 0.0
    with pytest.raises(ValueError):
        npm.optimizer.warmup_cosine(1.0, 5, 5)


class RecordingComm:
    """A communicator whose ``active`` is true and which only records: one rank, nothing to add."""
    active = True
    rank, size = 0, 1

    def __init__(self, sim):
        self.sim = sim

    def allreduce_async(self, flat, op):
        self.sim.calls.append('allreduce')

    def wait(self):
        self.sim.calls.append('comm_wait')

    def allreduce_scalar(self, value, op):
        return value

    def barrier(self):
        pass


def test_every_all_reduce_precedes_the_first_sum(npm):
    from np_modeling_amd import parallel
    lm = MC.make_lm(npm)
    parallel.set_communicator(RecordingComm(npm.sim))
    opt = AC.watching(npm, 1e-2, clip_norm=1.0)
    start = len(npm.sim.calls)
    AC.train(npm, lm, opt, 1)
    calls = npm.sim.calls[start:]
    assert calls.count('allreduce') >= 1 and 'npm_sumsq_ranges' in calls
    first_sum = calls.index('npm_sumsq_ranges')
    assert max(i for i, c in enumerate(calls) if c == 'allreduce') < first_sum
    assert max(i for i, c in enumerate(calls) if c == 'comm_wait') < first_sum


def test_trainer_calls_apply_once_per_step_and_leaves_sgd_as_it_was(npm):
    lm = MC.make_lm(npm)
    opt = AC.watching(npm, 1e-2, clip_norm=1.0)
    AC.train(npm, lm, opt, 4)
    assert opt.applies == 4
    with open(os.path.join(ROOT, 'tests', 'golden', 'trainer_sgd_calls.json')) as f:
        recorded = json.load(f)['calls']
    lm = MC.make_lm(npm)
    start = len(npm.sim.calls)
    AC.train(npm, lm, npm.optimizer.SGDOptimizer(0.02), 2)
    assert npm.sim.calls[start:] == recorded and len(recorded) > 100
    assert not hasattr(npm.optimizer.SGDOptimizer(0.1), 'apply') and not hasattr(npm.optimizer.AdamOptimizer(0.1), 'apply')


def test_the_new_kernels_spill_nothing(built):
    """Code-object metadata of the four gfx950 kernels of csrc/npm_clip.hip (tools/kernel_meta.py): no spill, no scratch -- the
    ranges table is a kernel argument indexed at run time, which must stay scalar loads."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import kernel_meta
    meta = kernel_meta.kernel_metadata(os.path.join(os.path.dirname(built.LIB_PATH), 'npm_clip.o'))
    assert len(meta) == 4 and all(any(tag in name for name in meta) for tag in ('sumsq_tiles', 'sumsq_finish', 'clip_finish', 'adamw_kernel'))
    for name, m in meta.items():
        assert m['.vgpr_spill_count'] == 0 and m['.sgpr_spill_count'] == 0 and m['.private_segment_fixed_size'] == 0, (name, m)


def test_the_entry_points_are_declared_bound_and_not_part_of_the_simulator():
    """The name is from when the three were restated beside the simulator and therefore bound through ``_SPECIAL``; they are part
    of it now, and bound where every call that returns a status is."""
    import ctypes
    from np_modeling_amd import _C
    P = ctypes.c_void_p
    D = ctypes.c_double
    assert _C.SIGNATURES['npm_sumsq_ranges'] == [ctypes.POINTER(_C.npm_ranges), P]
    assert _C.SIGNATURES['npm_clip_finish'] == [P, D]
    assert _C.SIGNATURES['npm_adamw_step'] == [P, P, P, P, ctypes.c_size_t, D, D, D, D, ctypes.c_int, D, P]
    assert not {'npm_sumsq_ranges', 'npm_clip_finish', 'npm_adamw_step'} & set(_C._SPECIAL)
    header = open(os.path.join(ROOT, 'include', 'npm_hip.h')).read()
    assert '#define NPM_SUMSQ_TILE %d' % _C.SUMSQ_TILE in header and _C.SUMSQ_TILE == AR.TILE == 256 * 64
    assert '#define NPM_SUMSQ_MAX_RANGES %d' % _C.SUMSQ_MAX_RANGES in header
    assert ctypes.sizeof(_C.npm_ranges) == 32 * 8 + 32 * 8 + 8 and _C.npm_ranges.count.offset == 512
    assert '#define NPM_ABI_VERSION 2 ' in header
    assert OC.BAD_ARGUMENT == 10002
