"""GPU: npm_softmax_xent_rows through the C ABI and ``loss.SoftmaxCrossEntropyLoss`` on the device.

Bounds.  Every case of tests/xent_cases.py is held to the three bounds include/npm_hip.h derives for the entry point (row_loss,
row_lse, gradient; tests/xent_reference.py ``bounds`` evaluates them in fp64 from the same inputs) -- derived from the kernel's
operation count and the accuracy of expf, not measured; each case prints its worst |device - fp64| / bound.  Independently the
gradient of every row meets the project's parity contract against fp64 (NPM_PARITY_SCALED_F32 over the row, NPM_PARITY_REL_F32 on
the elements of at least 0.1 of the row's maximum; 2^-50, the reference's own rounding, is allowed on top, for rows whose exact
gradient is zero).  Everything the contract calls reproducible is compared as uint32.  Every buffer the kernel writes lies between
guard words and inside pitch padding filled with a sentinel, all of which are checked after every call.

Every test here needs npm_softmax_xent_rows or ``SoftmaxCrossEntropyLoss``: none passes on the parent commit."""

import ctypes as C

import numpy as np
import pytest

import xent_cases as XC
import xent_reference as XR

pytestmark = pytest.mark.gpu

GUARD = 8                                                       # floats: 32 bytes, so the alignment behind it is the allocation's
SENTINEL = np.array([0x5A5A5A5A], dtype=np.uint32).view(np.float32)[0]
WORST = {}                                                      # case -> (loss, lse, gradient): worst fraction of the bound


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


class Out:
    def __init__(self, row_loss, lse, grad, loss_sum, kernel):
        self.row_loss, self.lse, self.grad, self.loss_sum, self.kernel = row_loss, lse, grad, loss_sum, kernel

    def same_bits(self, other, rows=slice(None), other_rows=slice(None)):
        same = np.array_equal(_bits(self.row_loss[rows]), _bits(other.row_loss[other_rows])) \
            and np.array_equal(_bits(self.lse[rows]), _bits(other.lse[other_rows]))
        if self.grad is not None and other.grad is not None:
            same = same and np.array_equal(_bits(self.grad[rows]), _bits(other.grad[other_rows]))
        return same


def _padded(z, pad, offset):
    """(host buffer with guards, pitch padding and the offset in front, all sentinel outside the rows; first float of row 0; pitch)"""
    rows, vocab = z.shape
    ld = vocab + pad
    first = GUARD + offset
    host = np.full(first + rows * ld + GUARD, SENTINEL, dtype=np.float32)
    body = host[first:first + rows * ld].reshape(rows, ld)
    body[:, :vocab] = z
    return host, first, ld


def _untouched_outside(host_after, first, rows, vocab, ld, what):
    sentinel = _bits(np.array([SENTINEL]))[0]
    bits = _bits(host_after)
    assert (bits[:first] == sentinel).all(), what + ': guard in front'
    assert (bits[first + rows * ld:] == sentinel).all(), what + ': guard behind'
    assert (bits[first:first + rows * ld].reshape(rows, ld)[:, vocab:] == sentinel).all(), what + ': pitch padding'


def run(z, t, smoothing=0.0, grad_scale=1.0, pad=0, offset=0, grad='fresh'):
    """One call of npm_softmax_xent_rows.  grad: 'fresh' (its own buffer, laid out like the logits), 'inplace' or 'none'."""
    from np_modeling_amd import _C, device as D
    z = np.asarray(z, dtype=np.float32)
    rows, vocab = z.shape
    host, first, ld = _padded(z, pad, offset)
    logits = D.from_host(host)
    ids = D.ids_from_host(np.asarray(t, dtype=np.int32))
    per_row = D.from_host(np.full(3 * GUARD + 2 * rows, SENTINEL, dtype=np.float32))
    dev_grad = None
    if grad == 'fresh':
        dev_grad = D.from_host(np.full(host.size, SENTINEL, dtype=np.float32))
    elif grad == 'inplace':
        dev_grad = logits
    total = C.c_double(np.nan)
    lib = _C.lib()
    _C.check(lib.npm_softmax_xent_rows(logits.ptr + 4 * first, ld, ids.ptr, rows, vocab, smoothing, grad_scale,
                                       None if dev_grad is None else dev_grad.ptr + 4 * first, ld,
                                       per_row.ptr + 4 * GUARD, per_row.ptr + 4 * (2 * GUARD + rows), C.byref(total)),
             'npm_softmax_xent_rows')
    kernel = _C.last_xent_kernel()
    vec = (logits.ptr + 4 * first) % 16 == 0 and ld % 4 == 0
    assert kernel == f'{XC.instance_of(vocab)} V={vocab} grad={int(grad != "none")} inplace={int(grad == "inplace")} ' \
                     f'vec={int(vec)} nt={int(4 * rows * vocab >= 32 << 20)}', kernel
    after = per_row.numpy()
    sentinel = _bits(np.array([SENTINEL]))[0]
    for lo, hi in ((0, GUARD), (GUARD + rows, 2 * GUARD + rows), (2 * GUARD + 2 * rows, 3 * GUARD + 2 * rows)):
        assert (_bits(after[lo:hi]) == sentinel).all(), 'guards of row_loss / row_lse'
    row_loss, lse = after[GUARD:GUARD + rows].copy(), after[2 * GUARD + rows:2 * GUARD + 2 * rows].copy()
    logits_after = logits.numpy()
    _untouched_outside(logits_after, first, rows, vocab, ld, 'logits')
    if grad != 'inplace':
        assert np.array_equal(_bits(logits_after), _bits(host)), 'the logits were written'
    out_grad = None
    if dev_grad is not None:
        grad_after = logits_after if grad == 'inplace' else dev_grad.numpy()
        _untouched_outside(grad_after, first, rows, vocab, ld, 'gradient')
        out_grad = grad_after[first:first + rows * ld].reshape(rows, ld)[:, :vocab].copy()
    return Out(row_loss, lse, out_grad, total.value, kernel)


def parity_contract(got, ref):
    """The project's contract (include/npm_hip.h NPM_PARITY_*), row by row, on the rows whose reference is finite."""
    from np_modeling_amd import _C
    rel_bound, scaled_bound = _C.parity_bounds()['f32']
    worst_rel = worst_scaled = 0.0
    for g, r in zip(np.asarray(got, dtype=np.float64), ref):
        if not np.isfinite(r).all():
            continue
        top = np.abs(r).max()
        err = np.abs(g - r)
        assert (err <= scaled_bound * top + 2.0 ** -50).all(), ('scaled', float(err.max()), float(top))
        big = np.abs(r) >= 0.1 * top
        assert (err[big] <= rel_bound * np.abs(r[big]) + 2.0 ** -50).all(), ('rel', float((err[big] / np.abs(r[big])).max()))
        if top > 2.0 ** -40:
            worst_scaled, worst_rel = max(worst_scaled, float(err.max() / top)), max(worst_rel, float((err[big] / np.abs(r[big])).max()))
    return worst_rel, worst_scaled


def _scale_of(case):
    live = max(int((XC.data(case)[1] >= 0).sum()), 1)
    return (1.0, 1.0 / live)[case.index % 2]


# ---- every case against the fp64 reference -----------------------------------------------------------------------------------

@pytest.mark.parametrize('case', XC.CASES, ids=XC.case_id)
def test_every_case_is_within_the_derived_bound_of_the_fp64_reference(npm, case):
    z, t = XC.data(case)
    scale = _scale_of(case)
    got = run(z, t, case.smoothing, scale, case.pad, case.offset)
    assert got.kernel.startswith(XC.instance_of(case.vocab) + ' ')
    ref = XR.reference(z, t, case.smoothing, scale)
    b_loss, b_lse, b_grad = XR.bounds(z, t, case.smoothing, scale)
    fractions = (XR.worst_fraction(got.row_loss, ref.row_loss, b_loss), XR.worst_fraction(got.lse, ref.lse, b_lse),
                 XR.worst_fraction(got.grad, ref.grad, b_grad))
    rel, scaled = parity_contract(got.grad, ref.grad)
    print(f'{XC.case_id(case)}: worst |device - fp64| / bound: loss {fractions[0]:.3f} lse {fractions[1]:.3f} gradient {fractions[2]:.3f}; '
          f'parity rel {rel:.2e} scaled {scaled:.2e}')
    assert max(fractions) <= 1.0, fractions
    # the sum: the fp64 sum of the fp32 row losses, so within the rows' bounds of the reference's sum
    if np.isfinite(ref.loss_sum):
        assert abs(got.loss_sum - ref.loss_sum) <= b_loss.sum() + 2.0 ** -50 * np.abs(ref.row_loss).sum()
        assert got.loss_sum == pytest.approx(got.row_loss.astype(np.float64).sum(), rel=2.0 ** -45, abs=0.0)
    else:
        assert np.isnan(got.loss_sum) == np.isnan(ref.loss_sum) and (np.isnan(ref.loss_sum) or got.loss_sum == ref.loss_sum)
    WORST[case] = fractions
    for k, what in enumerate(('row_loss', 'row_lse', 'gradient')):      # the last case's lines are the session's worst, for DESIGN.md
        top = max(WORST, key=lambda c: WORST[c][k])
        print(f'  worst so far, {what}: {WORST[top][k]:.3f} at {XC.case_id(top)} ({len(WORST)} cases)')


def test_every_instance_of_the_table_ran(npm):
    """Each case asserts (in ``run``) that the instance the table names is the one npm_last_xent_kernel reports; here: the cases
    name every instance of the table, on the 16-byte and on the scalar path."""
    named = {(XC.instance_of(c.vocab), c.pad == 1 or c.offset == 1) for c in XC.CASES if c.ignore != 'all'}
    assert named == {(name, scalar) for name, _, _ in XC.INSTANCES for scalar in (False, True)}
    for name, low, _ in XC.INSTANCES:                           # and the first vocabulary of each instance reports that name
        got = run(np.zeros((1, low), dtype=np.float32), [0])
        assert got.kernel.split()[0] == name
        assert got.row_loss[0] == np.float32(np.log(low))


# ---- bitwise properties ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', XC.CASES, ids=XC.case_id)
def test_launches_inplace_and_the_loss_alone_give_the_same_bits(npm, case):
    z, t = XC.data(case)
    first = run(z, t, case.smoothing, 0.5, case.pad, case.offset)
    again = run(z, t, case.smoothing, 0.5, case.pad, case.offset)
    assert first.same_bits(again)
    assert first.loss_sum == again.loss_sum or (np.isnan(first.loss_sum) and np.isnan(again.loss_sum))
    over = run(z, t, case.smoothing, 0.5, case.pad, case.offset, grad='inplace')
    assert first.same_bits(over)
    alone = run(z, t, case.smoothing, 0.5, case.pad, case.offset, grad='none')
    assert alone.grad is None and first.same_bits(alone)
    assert first.loss_sum == alone.loss_sum or np.isnan(first.loss_sum)
    ignored = np.asarray(t) < 0
    assert not first.row_loss[ignored].any() and not _bits(first.grad[ignored]).any()       # exact +0.0
    assert np.isnan(first.lse[ignored]).all()


@pytest.mark.parametrize('case', [c for c in XC.CASES if c.rows == 64 and c.ignore != 'all'], ids=XC.case_id)
def test_a_row_alone_is_the_row_inside_the_batch(npm, case):
    z, t = XC.data(case)
    whole = run(z, t, case.smoothing, 0.25, case.pad, case.offset)
    for r in (0, 1, 2, 3, 37, 63):
        single = run(z[r:r + 1], t[r:r + 1], case.smoothing, 0.25, case.pad, case.offset)
        assert single.same_bits(whole, other_rows=slice(r, r + 1)), r


@pytest.mark.parametrize('vocab', [3, 65, 1000, 1026, 8191, 8194, 32768, 40003])
def test_pitch_and_alignment_change_no_bit(npm, vocab):
    rng = np.random.default_rng(vocab)
    z = (4 * rng.standard_normal((5, vocab))).astype(np.float32)
    t = rng.integers(0, vocab, size=5)
    tight = run(z, t, 0.1, 1.0, 0, 0)
    for pad, offset in ((4, 0), (1, 0), (0, 1), (3, 1), (4 - vocab % 4, 0)):
        other = run(z, t, 0.1, 1.0, pad, offset)
        assert tight.same_bits(other), (pad, offset)
        assert tight.loss_sum == other.loss_sum


@pytest.mark.parametrize('case', [c for c in XC.CASES if c.ignore in ('first', 'last') and c.rows > 1], ids=XC.case_id)
def test_an_ignored_row_is_not_read(npm, case):
    z, t = XC.data(case)
    clean = run(z, t, case.smoothing, 1.0, case.pad, case.offset)
    dirty = z.copy()
    dirty[np.asarray(t) < 0] = np.nan
    assert clean.same_bits(run(dirty, t, case.smoothing, 1.0, case.pad, case.offset))
    assert np.isfinite(clean.loss_sum) or case.smoothing != 0.0


# ---- the non-finite contract -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('smoothing', [0.0, 0.1])
@pytest.mark.parametrize('vocab, pad', [(65, 1), (1000, 0), (1026, 4), (9000, 0), (40003, 1)])
def test_non_finite_rows_and_targets(npm, vocab, pad, smoothing):
    rng = np.random.default_rng(vocab + 7)
    z = (3 * rng.standard_normal((5, vocab))).astype(np.float32)
    t = rng.integers(0, vocab, size=5).astype(np.int32)
    base = run(z, t, smoothing, 1.0, pad)
    others = [0, 1, 3, 4]

    def variant(edit, target=None):
        zz, tt = z.copy(), t.copy()
        edit(zz[2])
        if target is not None:
            tt[2] = target
        got = run(zz, tt, smoothing, 1.0, pad)
        assert got.same_bits(base, rows=others, other_rows=others), 'a neighbouring row changed'
        over = run(zz, tt, smoothing, 1.0, pad, grad='inplace')
        assert got.same_bits(over)
        return got, XR.reference(zz, tt, smoothing, 1.0), (zz, tt)

    def all_nan(got):
        assert np.isnan(got.row_loss[2]) and np.isnan(got.lse[2]) and np.isnan(got.grad[2]).all() and np.isnan(got.loss_sum)

    spot = vocab // 2
    all_nan(variant(lambda row: row.__setitem__(spot, np.nan))[0])
    all_nan(variant(lambda row: row.__setitem__(vocab - 1, np.inf))[0])
    all_nan(variant(lambda row: row.__setitem__(slice(None), -np.inf))[0])
    all_nan(variant(lambda row: None, target=vocab)[0])                             # t >= V: no access outside the row
    all_nan(variant(lambda row: None, target=2 ** 31 - 1)[0])
    # a -inf target logit: the loss is +inf, the gradient of the masked target is 0, the rest as the formula says
    got, ref, (zz, tt) = variant(lambda row: row.__setitem__(int(t[2]), -np.inf))
    assert got.row_loss[2] == np.inf and ref.row_loss[2] == np.inf and got.loss_sum == np.inf
    assert got.grad[2, t[2]] == 0.0 and np.isfinite(got.lse[2])
    b_loss, b_lse, b_grad = XR.bounds(zz, tt, smoothing, 1.0)
    assert XR.worst_fraction(got.lse, ref.lse, b_lse) <= 1.0 and XR.worst_fraction(got.grad, ref.grad, b_grad) <= 1.0
    # masked tokens elsewhere: 0 in the sum, gradient exactly 0; with smoothing the loss is +inf
    got, ref, (zz, tt) = variant(lambda row: row.__setitem__(slice(0, int(t[2])), -np.inf) if t[2] > 0 else row.__setitem__(slice(1, 2), -np.inf))
    masked = np.isneginf(zz[2])
    assert masked.any() and not _bits(got.grad[2][masked]).any()
    assert got.row_loss[2] == np.inf if smoothing else np.isfinite(got.row_loss[2])
    b_loss, b_lse, b_grad = XR.bounds(zz, tt, smoothing, 1.0)
    assert max(XR.worst_fraction(got.row_loss, ref.row_loss, b_loss), XR.worst_fraction(got.lse, ref.lse, b_lse),
               XR.worst_fraction(got.grad, ref.grad, b_grad)) <= 1.0


def test_bad_arguments_are_refused_before_a_launch(npm):
    from np_modeling_amd import _C, device as D
    z, ids, out = D.from_host(np.zeros((4, 8), dtype=np.float32)), D.ids_from_host(np.arange(4)), D.empty([2, 4])
    total = C.c_double(7.0)
    lib = _C.lib()

    def call(grad_ptr=None, ldd=8, e=0.0, ld=8, rows=3, vocab=8, logits=z.ptr, sum_ref=C.byref(total)):
        return lib.npm_softmax_xent_rows(logits, ld, ids.ptr, rows, vocab, e, 1.0, grad_ptr, ldd, out.ptr, out.ptr + 16, sum_ref)

    bad = 10002
    assert call(z.ptr + 32) == bad and b'bad argument' in lib.npm_last_error()           # shifted by one row
    assert call(z.ptr + 4 * 23) == bad                                                  # the last float of the logits
    assert call(z.ptr, ldd=9) == bad                                                    # in place with another pitch
    assert call(e=1.0) == bad and call(e=-0.5) == bad and call(e=float('nan')) == bad
    assert call(ld=7) == bad and call(vocab=0) == bad and call(rows=-1) == bad and call(sum_ref=None) == bad
    assert call(logits=None) == bad and call(z.ptr, ldd=7) == bad
    assert total.value == 7.0
    assert call(rows=0, logits=None) == 0 and total.value == 0.0 and _C.last_xent_kernel() == 'xent_none rows=0'
    assert call(z.ptr + 4 * 24) == 0                                                    # adjacent, not overlapping
    assert total.value == pytest.approx(3 * np.log(8), rel=1e-6)


# ---- the nontemporal variants: a tensor of 32 MB --------------------------------------------------------------------------------

@pytest.mark.parametrize('rows, vocab', [(8192, 1024), (1024, 8192), (256, 32768), (208, 40336)])
def test_the_nontemporal_variant_gives_the_bits_of_the_default_policy(npm, rows, vocab):
    from np_modeling_amd import _C
    rng = np.random.default_rng(rows)
    z = (2 * rng.standard_normal((rows, vocab))).astype(np.float32)
    t = rng.integers(-1, vocab, size=rows)
    assert 4 * rows * vocab >= 32 << 20
    streamed = run(z, t, 0.0, 1.0 / rows)
    assert streamed.kernel.endswith('nt=1')
    inplace = run(z, t, 0.0, 1.0 / rows, grad='inplace')
    _C.check(_C.lib().npm_set_tuning(12, 0), 'npm_set_tuning')                           # NPM_TUNE_STREAM_NT
    try:
        plain = _run_without_name_check(z, t, 1.0 / rows)
    finally:
        _C.check(_C.lib().npm_set_tuning(12, 1), 'npm_set_tuning')
    assert plain.kernel.endswith('nt=0') and streamed.same_bits(plain) and streamed.same_bits(inplace)
    some = np.r_[0:3, rows - 3:rows]
    ref = XR.reference(z[some], t[some], 0.0, 1.0 / rows)
    b_loss, b_lse, b_grad = XR.bounds(z[some], t[some], 0.0, 1.0 / rows)
    assert max(XR.worst_fraction(streamed.row_loss[some], ref.row_loss, b_loss), XR.worst_fraction(streamed.lse[some], ref.lse, b_lse),
               XR.worst_fraction(streamed.grad[some], ref.grad, b_grad)) <= 1.0


def _run_without_name_check(z, t, scale):
    """``run`` for a call whose nt flag does not follow from the size (the knob is off)."""
    from np_modeling_amd import _C, device as D
    rows, vocab = z.shape
    logits, ids, per_row, grad = D.from_host(z), D.ids_from_host(np.asarray(t, dtype=np.int32)), D.empty([2, rows]), D.empty([rows, vocab])
    total = C.c_double()
    _C.check(_C.lib().npm_softmax_xent_rows(logits.ptr, vocab, ids.ptr, rows, vocab, 0.0, scale, grad.ptr, vocab, per_row.ptr,
                                            per_row.ptr + 4 * rows, C.byref(total)), 'npm_softmax_xent_rows')
    both = per_row.numpy()
    return Out(both[0], both[1], grad.numpy(), total.value, _C.last_xent_kernel())


# ---- against shipped code ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('vocab', [257, 5000, 32768, 40003])
def test_row_loss_is_minus_the_log_probability_sampling_reports(npm, vocab):
    import logits_reference as LR
    from np_modeling_amd import device as D, loss, sampling
    rng = np.random.default_rng(vocab)
    z = (5 * rng.standard_normal((6, vocab))).astype(np.float32)
    z[4, 10:200] = -np.inf
    t = rng.integers(0, vocab, size=6)
    t[2], t[4] = -1, 5                                          # ignored; outside the masked block
    logits = D.from_host(z)
    xent = loss.SoftmaxCrossEntropyLoss(reduction='sum')
    xent.forward(logits, t, need_grad=False)
    theirs = sampling.logprobs(logits, ids=t)
    live = t >= 0
    want = XR.reference(z, t).row_loss
    b_loss, b_lse, _ = XR.bounds(z, t)
    mine, chosen = xent.row_loss.numpy().astype(np.float64), theirs.chosen.astype(np.float64)
    assert (np.abs(mine[live] + chosen[live]) <= b_loss[live] + LR.eps(want[live], vocab)).all()
    assert (np.abs(xent.lse.numpy()[live].astype(np.float64) - theirs.lse[live]) <= b_lse[live] + LR.eps(XR.reference(z, t).lse[live], vocab)).all()
    assert mine[2] == 0.0 and np.isnan(chosen[2])


def test_todays_composition_agrees_where_it_can_be_run(npm):
    """Softmax + CrossEntropyLoss over one-hot float targets, sum reduction, logits of scale 1 (no probability underflows)."""
    from np_modeling_amd import _C, device as D, layers, loss
    rng = np.random.default_rng(11)
    rows, vocab = 37, 300
    z = rng.standard_normal((rows, vocab)).astype(np.float32)
    t = rng.integers(0, vocab, size=rows)
    softmax, old = layers.activations.Softmax(), loss.CrossEntropyLoss()
    old_value = old(softmax(D.from_host(z)), np.eye(vocab, dtype=np.float32)[t])
    old_grad = softmax(old(backprop=True), backprop=True).numpy()
    new = loss.SoftmaxCrossEntropyLoss(reduction='sum')
    new_value = new(D.from_host(z), t)
    rel, scaled = _C.parity_bounds()['f32']
    assert abs(new_value - old_value) <= rel * abs(old_value)
    parity_contract(new(backprop=True).numpy(), old_grad.astype(np.float64))
    ref = XR.reference(z, t)
    assert abs(new_value - ref.loss_sum) <= abs(old_value - ref.loss_sum) + 2.0 ** -24 * ref.loss_sum      # and no further from fp64


# ---- the loss class on the device --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('inplace', [False, True])
def test_the_loss_class_on_the_device(npm, inplace):
    from np_modeling_amd import device as D, loss
    rng = np.random.default_rng(3)
    z = (2 * rng.standard_normal((3, 7, 1500))).astype(np.float32)
    t = rng.integers(0, 1500, size=(3, 7))
    t[1, 4:] = -1
    t[2, 6] = 1500                                              # beyond the vocabulary: legal as the pad id below
    xent = loss.SoftmaxCrossEntropyLoss(ignore_index=1500, label_smoothing=0.1, inplace=inplace)
    logits = D.from_host(z)
    value = xent.forward(logits, np.where(t == -1, 1500, t))
    ids = np.where(t == 1500, -1, t).reshape(-1)
    count = int((ids >= 0).sum())
    ref = XR.reference(z.reshape(21, 1500), ids, 0.1, 1.0 / count)
    b_loss, b_lse, b_grad = XR.bounds(z.reshape(21, 1500), ids, 0.1, 1.0 / count)
    assert xent.count == count == 17
    assert abs(value - ref.loss_sum / count) <= b_loss.sum() / count + 1e-15
    grad = xent.backward()
    assert (grad is logits) == inplace and grad.shape == (3, 7, 1500)
    assert XR.worst_fraction(grad.numpy().reshape(21, 1500), ref.grad, b_grad) <= 1.0
    assert XR.worst_fraction(xent.row_loss.numpy().reshape(21), ref.row_loss, b_loss) <= 1.0
    assert XR.worst_fraction(xent.lse.numpy().reshape(21), ref.lse, b_lse) <= 1.0
    # evaluation: the same loss, no gradient; an IdBuffer: counted once, an id beyond the vocabulary is NaN and nothing faults
    quiet = loss.SoftmaxCrossEntropyLoss(label_smoothing=0.1)
    assert quiet.forward(D.from_host(z), ids.reshape(3, 7), need_grad=False) == value
    with pytest.raises(RuntimeError):
        quiet.backward()
    wild = ids.copy()
    wild[5] = 1500
    out = loss.SoftmaxCrossEntropyLoss(reduction='sum')
    assert np.isnan(out.forward(D.from_host(z), D.ids_from_host(wild.reshape(3, 7))))
    got = out.backward().numpy().reshape(21, 1500)
    assert np.isnan(got[5]).all() and np.isfinite(np.delete(got, 5, axis=0)).all() and np.isnan(out.row_loss.numpy().reshape(21)[5])
