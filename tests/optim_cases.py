"""TEST INFRASTRUCTURE: the cases and checks of the optimizer, loss and dropout kernels (csrc/npm_optim.hip), written once and run
through whatever library ``np_modeling_amd._C`` holds: the host simulator in tests/test_optim_host.py, libnpm_hip.so in
tests/test_gpu_optim.py.  Models and bounds: tests/optim_reference.py.

Sizes come from the launch code: elementwise kernels and Adam run at most 4096 blocks of 256 threads, so their grid-stride pass
starts at 1 048 576 elements; the loss sums run at most 1024 blocks, so theirs starts at 262 144.  Every output buffer, the moments
and the byte mask carry GUARD sentinel elements behind them (and in front of an offset view), checked after the call.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

import optim_reference as R

EW_SEAM = 4096 * 256
SUM_SEAM = 1024 * 256
GUARD = 96
SENTINEL = np.float32(-77.25)
SENTINEL64 = np.float64(-77.25)
SENTINEL_BYTE = 0xA5
BAD_ARGUMENT, UNSUPPORTED = 10002, 10003


def sizes(seam: int) -> list:
    return [1, 3, 255, 256, 257, 1023, seam - 1, seam, seam + 257]


UNALIGNED_N = 997                       # with flat_view offsets 1 and 3, as test_elementwise_unaligned_views


# ---- buffers with guards ----------------------------------------------------------------------------------------------------------------
class F32:
    """n floats at ``offset`` floats into a sentinel-filled device array with GUARD more behind."""

    def __init__(self, npm, n, offset=0, host=None):
        D = npm.device
        self.n, self.offset = int(n), int(offset)
        self.base = D.full([self.offset + self.n + GUARD], float(SENTINEL))
        self.view = self.base.flat_view(self.offset, [self.n])
        self.ptr = self.view.ptr
        if host is not None:
            self.view.set(host)

    def numpy(self):
        return self.view.numpy()

    def guards_intact(self):
        whole = self.base.numpy()
        return bool((whole[:self.offset] == SENTINEL).all() and (whole[self.offset + self.n:] == SENTINEL).all())


class Raw:
    """``count`` elements of ``dtype`` (uint8 or float64) at byte offset ``offset`` inside a device.ByteBuffer, sentinels around."""

    def __init__(self, npm, dtype, count, offset=0, host=None):
        from np_modeling_amd import _C
        self._C, self.dtype = _C, np.dtype(dtype)
        self.count, self.offset = int(count), int(offset)
        self.sentinel = SENTINEL_BYTE if self.dtype == np.uint8 else SENTINEL64
        self.tail = GUARD * self.dtype.itemsize
        self.buf = npm.device.ByteBuffer(self.offset + self.count * self.dtype.itemsize + self.tail)
        self.ptr = self.buf.ptr + self.offset
        whole = np.full(self.buf.nbytes, SENTINEL_BYTE, dtype=np.uint8)
        body = np.full(self.count + GUARD, self.sentinel, dtype=self.dtype)
        if host is not None:
            body[:self.count] = host
        whole[self.offset:] = body.view(np.uint8)
        _C.check(_C.lib().npm_h2d(self.buf.ptr, whole.ctypes.data, whole.nbytes), 'npm_h2d')

    def _split(self):
        whole = self.buf.numpy()
        return whole[:self.offset], whole[self.offset:].view(self.dtype)

    def numpy(self):
        return self._split()[1][:self.count].copy()

    def guards_intact(self):
        front, body = self._split()
        return bool((front == SENTINEL_BYTE).all() and (body[self.count:] == self.sentinel).all())


def _lib():
    from np_modeling_amd import _C
    return _C, _C.lib()


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------
# (n, hyper, steps, (parameter offset, gradient offset) in floats, moment offset in doubles)
ADAM_CASES = [(n, R.DEFAULT_HYPER, (1, 2, 3), (0, 0), 0) for n in sizes(EW_SEAM)] + [
    (UNALIGNED_N, R.DEFAULT_HYPER, (1, 2, 3), (1, 3), 1),
    (4099, R.DEFAULT_HYPER, (1000,), (0, 0), 0),                     # step number 1000 from zero moments
    (4099, R.OTHER_HYPER, (1, 2, 3), (0, 0), 0),
]
ADAM_SEED = 20


def adam_case_id(case) -> str:
    n, hyper, steps, offsets, moff = case
    return f'n{n}-lr{hyper[0]:g}-steps{"_".join(map(str, steps))}-off{offsets[0]}{offsets[1]}'


def check_adam_case(npm, case, stepper=None) -> list:
    """Runs the case's steps in sequence; each step's model starts from the state read back after the step before, so nothing
    accumulates.  ``stepper(p, g, m, v, step, hyper) -> (p, m, v)`` replaces the library (the wrong models of the host tests).
    Returns [(step, near ties, near ties where the parameter differs)]."""
    n, hyper, steps, (poff, goff), moff = case
    rng = np.random.default_rng(ADAM_SEED + n)
    p0 = rng.standard_normal(n).astype(np.float32)
    p, m, v = p0, np.zeros(n), np.zeros(n)
    if stepper is None:
        _C, lib = _lib()
        dp = F32(npm, n, poff, p0)
        dm, dv = (Raw(npm, np.float64, n, 8 * moff, np.zeros(n)) for _ in range(2))
    used = []
    for step in steps:
        g = R.adam_gradient(rng, n)
        want = R.adam_model(p, g, m, v, step, hyper)
        if stepper is None:
            dg = F32(npm, n, goff, g)
            _C.check(lib.npm_adam_step(dp.ptr, dg.ptr, dm.ptr, dv.ptr, n, *hyper, step), 'npm_adam_step')
            got = dp.numpy(), dm.numpy(), dv.numpy()
            assert dp.guards_intact() and dm.guards_intact() and dv.guards_intact() and dg.guards_intact(), 'a guard was written'
            assert np.array_equal(R.bits(dg.numpy()), R.bits(g)), 'the gradient was written'
        else:
            got = stepper(p, g, m, v, step, hyper)
        exempt, differing = R.adam_check(*got, want, what=f'{adam_case_id(case)} step {step}')
        if step == 1:                                   # zero moments, zero gradient: no step at all
            zero = g == 0
            assert np.array_equal(R.bits(got[0][zero]), R.bits(p[zero])), 'g == 0 at step 1 changed the parameter'
        used.append((step, exempt, differing))
        p, m, v = got
    return used


def check_adam_golden(npm, golden) -> list:
    """tests/golden/adam_steps.npz: the reference's own AdamOptimizer, three steps at n = 1031.  Each step starts from the recorded
    state of the step before; the result is held to the RECORDED arrays under the near-tie rule."""
    _C, lib = _lib()
    hyper = tuple(float(h) for h in golden['hyper'])
    n = int(golden['p0'].size)
    p, m, v = golden['p0'], np.zeros(n), np.zeros(n)
    used = []
    for step in (1, 2, 3):
        g = golden[f'g{step}']
        model = R.adam_model(p, g, m, v, step, hyper)
        want = R.AdamStep(golden[f'p{step}'], golden[f'm{step}'], golden[f'v{step}'], model.d, model.upd)
        assert want.p.dtype == np.float32 and want.m.dtype == np.float64
        dp, dg = F32(npm, n, 0, p), F32(npm, n, 0, g)
        dm, dv = Raw(npm, np.float64, n, 0, m), Raw(npm, np.float64, n, 0, v)
        _C.check(lib.npm_adam_step(dp.ptr, dg.ptr, dm.ptr, dv.ptr, n, *hyper, step), 'npm_adam_step')
        used.append((step,) + R.adam_check(dp.numpy(), dm.numpy(), dv.numpy(), want, what=f'golden step {step}'))
        assert dp.guards_intact() and dm.guards_intact() and dv.guards_intact()
        p, m, v = want.p, want.m, want.v
    return used


def check_adam_optimizer_class(npm, n=EW_SEAM + 257, steps=2) -> list:
    """``AdamOptimizer.update`` on a device parameter: the class's own moments (read back through their pointers) and step count."""
    _C, lib = _lib()
    rng = np.random.default_rng(ADAM_SEED)
    p = rng.standard_normal(n).astype(np.float32)
    holder = type('Holder', (), {})()
    holder._w = var = npm.as_device(p)
    adam = npm.optimizer.AdamOptimizer(*R.DEFAULT_HYPER)
    m, v = np.zeros(n), np.zeros(n)
    used = []
    for step in range(1, steps + 1):
        g = R.adam_gradient(rng, n)
        adam.update(holder, '_w', npm.as_device(g))
        assert holder._w is var
        (count, moments), = adam._state.values()
        assert count == step + 1
        got_m, got_v = np.empty(n), np.empty(n)
        _C.check(lib.npm_d2h(got_m.ctypes.data, moments.first_ptr, 8 * n), 'npm_d2h')
        _C.check(lib.npm_d2h(got_v.ctypes.data, moments.second_ptr, 8 * n), 'npm_d2h')
        got_p = var.numpy()
        used.append((step,) + R.adam_check(got_p, got_m, got_v, R.adam_model(p, g, m, v, step), what=f'AdamOptimizer step {step}'))
        p, m, v = got_p, got_m, got_v
    return used


def encoder_adam_parameters(npm, coalesce: bool, steps=3) -> list:
    """Three Adam steps of a small encoder (d 8, 2 heads, hidden 20) with device.COALESCE_UPDATES as given; the 16 parameters."""
    from np_modeling_amd import parallel
    D = npm.device
    before, D.COALESCE_UPDATES = D.COALESCE_UPDATES, coalesce
    try:
        np.random.seed(3)
        rng = np.random.default_rng(3)
        layer = npm.layers.TransformerEncoder(num_heads=2, hidden_units=20, norm_first=True)
        x = rng.standard_normal([2, 5, 8]).astype(np.float32)
        dy = rng.standard_normal([2, 5, 8]).astype(np.float32)
        adam = npm.optimizer.AdamOptimizer(0.01)
        for _ in range(steps):
            layer(x)
            layer(dy, backprop=True, optimizer_=adam)
        assert parallel.GradScope.last['update_launches'] == (1 if coalesce else None), parallel.GradScope.last
        assert all(entry[0] == steps + 1 for entry in adam._state.values()) and len(adam._state) == 16
        return [np.asarray(p).copy() for p in parallel.parameters(layer)]
    finally:
        D.COALESCE_UPDATES = before


def check_encoder_adam_coalesced(npm):
    joined, single = encoder_adam_parameters(npm, True), encoder_adam_parameters(npm, False)
    assert len(joined) == len(single) == 16
    for a, b in zip(joined, single):
        assert np.array_equal(R.bits(a), R.bits(b))


# ---- losses ---------------------------------------------------------------------------------------------------------------------------
LOSS_CASES = [(n, (0, 0)) for n in sizes(SUM_SEAM)] + [(UNALIGNED_N, (1, 3))]
BWD_CASES = [(n, (0, 0, 0)) for n in sizes(EW_SEAM)] + [(UNALIGNED_N, (1, 3, 3)), (UNALIGNED_N, (0, 0, 1))]


def _loss(fn, y, t, n):
    from np_modeling_amd import _C
    out = C.c_double(float('nan'))
    _C.check(fn(y.ptr, t.ptr, n, C.byref(out)), 'loss')
    return out.value


def check_loss_sums(npm, case, mse=None, xent=None) -> dict:
    """npm_mse_fwd and npm_xent_fwd (one-hot and dense targets) against math.fsum; ``mse`` / ``xent`` (terms -> sum) replace the
    library.  Returns the errors in units of the bound."""
    n, (yoff, toff) = case
    rng = np.random.default_rng(n)
    used = {}
    lib = _lib()[1] if mse is None or xent is None else None
    y, t = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    if mse is None:
        got = _loss(lib.npm_mse_fwd, F32(npm, n, yoff, y), F32(npm, n, toff, t), n)
    else:
        got = mse(R.mse_terms(y, t)) / n
    used['mse'] = R.sum_check(got, R.mse_terms(y, t), n, what=f'mse n={n}')
    for onehot in (True, False):
        y, t = R.xent_inputs(rng, n, onehot)
        if xent is None:
            got = _loss(lib.npm_xent_fwd, F32(npm, n, yoff, y), F32(npm, n, toff, t), n)
        else:
            got = xent(R.xent_terms(y, t))
        used['xent onehot' if onehot else 'xent dense'] = R.sum_check(got, R.xent_terms(y, t), what=f'xent n={n} onehot={onehot}')
    return used


def check_loss_gradients(npm, case):
    """npm_mse_bwd is np.float32(2 / n) * (y - t), npm_xent_bwd is -t / y (t = 0 elements, y down to 1e-30), bit for bit."""
    _C, lib = _lib()
    n, (yoff, toff, ooff) = case
    rng = np.random.default_rng(n + 1)
    y, t = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    dy, dt, out = F32(npm, n, yoff, y), F32(npm, n, toff, t), F32(npm, n, ooff)
    _C.check(lib.npm_mse_bwd(dy.ptr, dt.ptr, out.ptr, n), 'npm_mse_bwd')
    assert np.array_equal(R.bits(out.numpy()), R.bits(np.float32(2.0 / n) * (y - t))) and out.guards_intact()
    y, t = R.xent_inputs(rng, n, False, y_min=1e-30)
    dy, dt, out = F32(npm, n, yoff, y), F32(npm, n, toff, t), F32(npm, n, ooff)
    _C.check(lib.npm_xent_bwd(dy.ptr, dt.ptr, out.ptr, n), 'npm_xent_bwd')
    assert np.array_equal(R.bits(out.numpy()), R.bits(-t / y)) and out.guards_intact()


# ---- npm_mask_scale -------------------------------------------------------------------------------------------------------------------
KEEPS = (1.0, 0.75, 0.1)
MASK_SCALE_CASES = [(n, keep, n % 4, (0, 0)) for n in sizes(EW_SEAM) for keep in (0.75,)] + [
    (UNALIGNED_N, keep, moff, offs) for keep in KEEPS for moff in range(4) for offs in ((0, 0), (1, 3))]


def check_mask_scale(npm, case):
    _C, lib = _lib()
    n, keep, moff, (xoff, yoff) = case
    rng = np.random.default_rng(n + moff)
    x = rng.standard_normal(n).astype(np.float32)
    mask = rng.choice(np.array([0, 1, 2, 255], dtype=np.uint8), size=n)
    dmask, dx, out = Raw(npm, np.uint8, n, moff, mask), F32(npm, n, xoff, x), F32(npm, n, yoff)
    _C.check(lib.npm_mask_scale(dx.ptr, dmask.ptr, out.ptr, n, keep), 'npm_mask_scale')
    assert np.array_equal(R.bits(out.numpy()), R.bits(R.mask_scale(x, mask, keep)))
    assert out.guards_intact() and dmask.guards_intact() and np.array_equal(dmask.numpy(), mask)


# ---- npm_dropout_philox ---------------------------------------------------------------------------------------------------------------
PHILOX_KEEPS = (1.0, 2.0 ** -33, 0.75, 0.1)           # threshold 2^32 (all kept), 0 (none kept), and two in between
SEEDS = (0xDEADBEEF12345678, 0xFFFFFFFF00000001)
OFFSETS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5)


def philox_grid() -> list:
    """(n, mask byte offset, x float offset, y float offset | None for the mask-only call, keep, seed, offset): every residue of
    n % 4 x every mask alignment x operand offsets that reach the 16-byte branch ((0, 0), and (4, 4) one vector further) and the
    scalar one, each keep probability; then the sizes below one block and around it; then seeds and offsets."""
    grid = []
    for n in (1024, 1025, 1026, 1027):
        for moff in range(4):
            for k, (xoff, yoff) in enumerate(((0, 0), (1, 0), (0, 2), (3, 3), (4, 4), (None, None))):
                for keep in PHILOX_KEEPS:
                    grid.append((n, moff, xoff, yoff, keep, SEEDS[(n + moff + k) & 1], OFFSETS[(moff + k) & 3]))
    for n in (1, 3, 255, 256, 257, 1023):
        grid += [(n, 0, 0, 0, 0.75, SEEDS[0], 1), (n, 0, None, None, 0.1, SEEDS[1], 0)]
    return grid


def run_philox(npm, n, moff, xoff, yoff, keep, seed, offset, x=None):
    _C, lib = _lib()
    dmask = Raw(npm, np.uint8, n, moff)
    if xoff is None:
        _C.check(lib.npm_dropout_philox(None, None, dmask.ptr, n, keep, seed, offset), 'npm_dropout_philox')
        out = None
    else:
        dx, out = F32(npm, n, xoff, x), F32(npm, n, yoff)
        _C.check(lib.npm_dropout_philox(dx.ptr, out.ptr, dmask.ptr, n, keep, seed, offset), 'npm_dropout_philox')
        assert out.guards_intact(), 'a guard behind y was written'
    assert dmask.guards_intact(), 'a guard around the mask was written'
    return dmask.numpy(), None if out is None else out.numpy()


def check_philox_case(npm, case, mask_model=None):
    """The mask is O.dropout_philox_mask (bytes 0 / 1) and y is np.where(mask, x / float32(keep), 0), bit for bit."""
    from oracle import np_oracle as O
    n, moff, xoff, yoff, keep, seed, offset = case
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    mask, y = run_philox(npm, n, moff, xoff, yoff, keep, seed, offset, x)
    want = (mask_model or O.dropout_philox_mask)(n, keep, seed, offset)
    assert np.array_equal(mask, want.astype(np.uint8)), case
    if keep == 1.0:
        assert mask.all()
    if keep == 2.0 ** -33:
        assert not mask.any()
    if y is not None:
        assert np.array_equal(R.bits(y), R.bits(R.mask_scale(x, want, keep))), case
        if keep == 1.0:
            assert np.array_equal(R.bits(y), R.bits(x))
        if keep == 2.0 ** -33:
            assert np.array_equal(R.bits(y), np.zeros(n, dtype=np.uint32))


def check_philox_offsets_differ(npm, n=1027):
    """Offsets 0, 2^32 - 1, 2^32 and 2^63 + 5 (both counter words, the top bit) and both seeds: eight different masks."""
    from oracle import np_oracle as O
    masks = {}
    for seed in SEEDS:
        for offset in OFFSETS:
            mask, _ = run_philox(npm, n, 0, None, None, 0.75, seed, offset)
            assert np.array_equal(mask, O.dropout_philox_mask(n, 0.75, seed, offset).astype(np.uint8)), (seed, offset)
            masks[seed, offset] = mask.tobytes()
    assert len(set(masks.values())) == len(SEEDS) * len(OFFSETS)


# ---- npm_fill_f64, argument checks --------------------------------------------------------------------------------------------------------
def check_fill_f64(npm):
    _C, lib = _lib()
    for n, off in ((1, 0), (257, 8), (EW_SEAM // 8 + 3, 0)):
        buf = Raw(npm, np.float64, n, off)
        assert lib.npm_fill_f64(buf.ptr, 0.0, 0) == 0 and (buf.numpy() == SENTINEL64).all()          # n = 0: accepted, nothing written
        assert lib.npm_fill_f64(None, 0.0, 0) == 0
        assert lib.npm_fill_f64(buf.ptr, 1.5, n) == UNSUPPORTED and (buf.numpy() == SENTINEL64).all()
        _C.check(lib.npm_fill_f64(buf.ptr, 0.0, n), 'npm_fill_f64')
        assert np.array_equal(R.bits(buf.numpy()), np.zeros(n, dtype=np.uint64)) and buf.guards_intact()
    assert lib.npm_fill_f64(None, 0.0, 4) == BAD_ARGUMENT


def check_arguments(npm):
    """Return codes only: a refused call launches nothing (the buffers keep their sentinels)."""
    _C, lib = _lib()
    n = 64
    p, g, y = F32(npm, n), F32(npm, n), F32(npm, n)
    m, v, mask = Raw(npm, np.float64, n), Raw(npm, np.float64, n), Raw(npm, np.uint8, n)
    hyper = R.DEFAULT_HYPER
    out = C.c_double(5.0)
    assert lib.npm_adam_step(p.ptr, g.ptr, m.ptr, v.ptr, n, *hyper, 0) == BAD_ARGUMENT            # step numbers start at 1
    assert lib.npm_adam_step(p.ptr, g.ptr, m.ptr, v.ptr, n, *hyper, -1) == BAD_ARGUMENT
    assert lib.npm_adam_step(p.ptr, g.ptr, None, v.ptr, n, *hyper, 1) == BAD_ARGUMENT
    for keep in (0.0, 1.5, -0.5):
        assert lib.npm_dropout_philox(p.ptr, y.ptr, mask.ptr, n, keep, 1, 0) == BAD_ARGUMENT, keep
    assert lib.npm_dropout_philox(p.ptr, None, mask.ptr, n, 0.5, 1, 0) == BAD_ARGUMENT            # x without y
    assert lib.npm_dropout_philox(None, y.ptr, mask.ptr, n, 0.5, 1, 0) == BAD_ARGUMENT
    assert lib.npm_dropout_philox(None, None, None, n, 0.5, 1, 0) == BAD_ARGUMENT
    assert lib.npm_mse_fwd(p.ptr, g.ptr, 0, C.byref(out)) == BAD_ARGUMENT and lib.npm_xent_fwd(p.ptr, g.ptr, 0, C.byref(out)) == BAD_ARGUMENT
    assert lib.npm_mse_fwd(p.ptr, None, n, C.byref(out)) == BAD_ARGUMENT and out.value == 5.0
    assert lib.npm_mask_scale(p.ptr, mask.ptr, y.ptr, n, 0.0) == BAD_ARGUMENT
    # n = 0 with NULL pointers: nothing to do, accepted
    assert lib.npm_adam_step(None, None, None, None, 0, *hyper, 1) == 0
    assert lib.npm_mse_bwd(None, None, None, 0) == 0 and lib.npm_xent_bwd(None, None, None, 0) == 0
    assert lib.npm_mask_scale(None, None, None, 0, 0.5) == 0 and lib.npm_dropout_philox(None, None, None, 0, 0.5, 1, 0) == 0
    for buf in (p, g, y):
        assert (buf.numpy() == SENTINEL).all() and buf.guards_intact()
    for buf in (m, v, mask):
        assert (buf.numpy() == buf.sentinel).all() and buf.guards_intact()
