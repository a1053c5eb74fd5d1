"""TEST INFRASTRUCTURE: NumPy models of what csrc/npm_optim.hip computes -- Adam, the two loss sums and their gradients, the mask
application and the Philox dropout mask -- and the checks that hold a result to them.  Shared by tests/test_optim_host.py (the
host simulator) and tests/test_gpu_optim.py (the library), through tests/optim_cases.py.

Adam.  ``adam_model`` is reference optimizer.py:53-67 restated for a float32 gradient: the two products (1 - beta) * g and
(1 - beta2) * g**2 are float32 (the gradient is a float32 array and Python scalars do not widen it), everything after them is
float64, and the parameter is rounded once (NumPy's ``f32 -= f64``).  tests/test_optim_host.py holds it bit for bit to the reference's
own class, and tests/golden/adam_steps.npz records that class's numbers.  Only fp32 / fp64 multiplies and adds produce the moments,
so a correct kernel gives their bits.  The parameter goes through an fp64 divide and a square root, which a device may round an
ulp off; that can move the float32 parameter only where the exact difference sits on a rounding boundary -- ``near_tie``.

Loss sums.  ``math.fsum`` over the float64 terms: the correctly rounded sum of the terms as float64 forms them.
"""

from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from oracle import np_oracle as O

DEFAULT_HYPER = (1e-2, 0.9, 0.999, 1e-7)            # lr, beta1, beta2, epsilon: the reference's defaults at lr 1e-2
OTHER_HYPER = (3e-4, 0.8, 0.99, 1e-8)
MAX_EXEMPT = 16                                     # near-tie elements a case may have (a condition on the data, not a tolerance)
SUM_BOUND = 1e-13                                   # |got - fsum| <= SUM_BOUND * sum |term| (derivation: tests/test_gpu_optim.py)


def bits(a) -> np.ndarray:
    """The array as unsigned integers of its own width: equality of these is equality of bits (signed zeros, NaNs)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def ordered(a) -> np.ndarray:
    """float32 -> int64 that increases with the value, one per representable number (distance = ulps)."""
    u = bits(np.asarray(a, dtype=np.float32)).astype(np.int64)
    return np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------
class AdamStep(NamedTuple):
    p: np.ndarray         # float32 parameter after the step
    m: np.ndarray         # float64 first moment after it
    v: np.ndarray         # float64 second moment
    d: np.ndarray         # the float64 difference p_before - step that p is the rounding of
    upd: np.ndarray       # the float64 step


def adam_model(p, g, m, v, step, hyper=DEFAULT_HYPER, variant=None) -> AdamStep:
    """One step from (p, m, v) with gradient g.  ``variant`` names one deliberate mistake (tests show each is caught):
    'round_step' rounds the step to float32 before subtracting, 'eps_outside' adds epsilon after the root, 'f32_moments' keeps the
    moments in float32, 'step_minus_1' corrects the bias with step - 1, 'f64_products' forms the two gradient products in float64."""
    lr, b1, b2, eps = (float(h) for h in hyper)
    p, g = np.asarray(p, dtype=np.float32), np.asarray(g, dtype=np.float32)
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(all='ignore'):
        if variant == 'f64_products':
            g64 = g.astype(np.float64)
            t1, t2 = (1 - b1) * g64, (1 - b2) * g64 ** 2
        else:
            t1 = (np.float32(1 - b1) * g).astype(np.float64)                  # float32 product
            t2 = (np.float32(1 - b2) * (g * g)).astype(np.float64)            # g * g rounded, then the product rounded
        nm, nv = b1 * m + t1, b2 * v + t2
        if variant == 'f32_moments':
            nm, nv = nm.astype(np.float32).astype(np.float64), nv.astype(np.float32).astype(np.float64)
        t = step - 1 if variant == 'step_minus_1' else step
        mh, vh = nm / (1 - b1 ** t), nv / (1 - b2 ** t)
        upd = lr * (mh / (np.sqrt(vh) + eps)) if variant == 'eps_outside' else lr * (mh / np.sqrt(vh + eps))
        if variant == 'round_step':
            upd = upd.astype(np.float32).astype(np.float64)
        d = p.astype(np.float64) - upd
        return AdamStep(d.astype(np.float32), nm, nv, d, upd)


def near_tie(d, upd) -> np.ndarray:
    """Elements whose float64 difference d lies within 2^-40 |step| + 2^-52 |d| of a float32 rounding boundary: the midpoint
    between float32(d) and its neighbour on d's side.  There -- and only there -- a divide or a root that is one fp64 ulp off
    (2^-52 of the step, with a wide margin for its propagation) may round the parameter to the other neighbour."""
    d, upd = np.asarray(d, dtype=np.float64), np.asarray(upd, dtype=np.float64)
    with np.errstate(all='ignore'):
        r = d.astype(np.float32)
        side = np.where(d > r.astype(np.float64), np.float32(np.inf), np.float32(-np.inf))
        mid = (r.astype(np.float64) + np.nextafter(r, side).astype(np.float64)) / 2       # exact in float64
        near = np.abs(d - mid) <= 2.0 ** -40 * np.abs(upd) + 2.0 ** -52 * np.abs(d)
    return near & (d != r.astype(np.float64)) & np.isfinite(d)


def adam_check(got_p, got_m, got_v, want: AdamStep, what='') -> tuple:
    """Moments bit-equal; parameters bit-equal except at near ties, where one float32 ulp either way is allowed; at most
    MAX_EXEMPT near ties.  Returns (near ties in the case, of those the number where the parameter differs)."""
    assert np.array_equal(bits(got_m), bits(want.m)), f'{what}: first moment differs in {int((bits(got_m) != bits(want.m)).sum())} elements'
    assert np.array_equal(bits(got_v), bits(want.v)), f'{what}: second moment differs in {int((bits(got_v) != bits(want.v)).sum())} elements'
    near = near_tie(want.d, want.upd)
    exempt = int(near.sum())
    assert exempt <= MAX_EXEMPT, f'{what}: {exempt} near-tie elements, more than {MAX_EXEMPT}: choose another seed'
    differs = bits(np.asarray(got_p, dtype=np.float32)) != bits(want.p)
    bad = differs & ~near
    assert not bad.any(), (f'{what}: parameter differs in {int(bad.sum())} of {bad.size} elements that are no near ties; first at '
                           f'{int(np.flatnonzero(bad)[0])}: got {np.asarray(got_p)[bad][0]!r}, want {want.p[bad][0]!r}')
    if differs.any():
        assert np.abs(ordered(np.asarray(got_p)[differs]) - ordered(want.p[differs])).max() <= 1, f'{what}: a near tie is off by more than one ulp'
    return exempt, int(differs.sum())


def adam_gradient(rng, n: int) -> np.ndarray:
    """Standard normal float32 with every 97th element exactly 0, a block of magnitudes 1e-20 and 1e19 (their squares are a float32
    denormal and 1e38) and a block of +-0."""
    g = rng.standard_normal(n).astype(np.float32)
    g[96::97] = 0.0
    if n >= 64:
        a, b = n // 4, n // 2
        g[a:a + 16] = np.tile(np.array([1e-20, -1e19, -1e-20, 1e19], dtype=np.float32), 4)
        g[b:b + 16] = np.tile(np.array([0.0, -0.0], dtype=np.float32), 8)
    elif n > 1:
        g[1:] = np.array([0.0, -0.0, 1e-20, -1e19] * 16, dtype=np.float32)[:n - 1]
    return g


# ---- loss sums ------------------------------------------------------------------------------------------------------------------------
def mse_terms(y, t) -> np.ndarray:
    d = np.asarray(y, dtype=np.float64) - np.asarray(t, dtype=np.float64)
    return d * d


def xent_terms(y, t) -> np.ndarray:
    return -(np.asarray(t, dtype=np.float64) * np.log(np.asarray(y, dtype=np.float64)))


def sum_check(got: float, terms: np.ndarray, divide_by: int = 1, what='') -> float:
    """|got - fsum(terms) / divide_by| <= SUM_BOUND * sum |terms| / divide_by; returns the error in units of the bound."""
    ref, scale = math.fsum(terms.tolist()), math.fsum(np.abs(terms).tolist())
    err, bound = abs(got - ref / divide_by), SUM_BOUND * scale / divide_by
    assert err <= bound, f'{what}: |{got!r} - {ref / divide_by!r}| = {err:.3e} > {bound:.3e}'
    return err / bound if bound else 0.0


def pairwise_f32_sum(terms: np.ndarray) -> float:
    """A deliberate mistake: the terms accumulated pairwise in float32."""
    a = np.asarray(terms).astype(np.float32)
    while a.size > 1:
        if a.size & 1:
            a = np.concatenate([a, np.zeros(1, dtype=np.float32)])
        a = a[0::2] + a[1::2]
    return float(a[0])


def xent_inputs(rng, n: int, onehot: bool, y_min: float = 1e-6):
    """y log-uniform in [y_min, 1] with both ends present; targets one-hot over rows of 32, or dense uniform with zeros."""
    y = np.exp(rng.uniform(np.log(y_min), 0.0, size=n)).astype(np.float32).clip(np.float32(y_min), np.float32(1.0))
    y[0] = 1.0
    if n > 1:
        y[-1] = y_min
    if onehot:
        t = (np.arange(n) % 32 == np.repeat(rng.integers(0, 32, size=(n + 31) // 32), 32)[:n]).astype(np.float32)
    else:
        t = rng.uniform(0.0, 1.0, size=n).astype(np.float32)
        t[::5] = 0.0
    return y, t


# ---- masks ---------------------------------------------------------------------------------------------------------------------------
def mask_scale(x, mask, keep) -> np.ndarray:
    with np.errstate(all='ignore'):
        return np.where(np.asarray(mask) != 0, np.asarray(x, dtype=np.float32) / np.float32(keep), np.float32(0)).astype(np.float32)


def philox_threshold(keep_prob: float) -> int:
    scaled = float(np.float32(keep_prob)) * 4294967296.0
    return 4294967296 if scaled >= 4294967296.0 else int(scaled)


def dropout_philox_mask_range(first: int, count: int, keep_prob: float, seed: int, offset: int, swap_offset_halves: bool = False) -> np.ndarray:
    """``O.dropout_philox_mask`` for elements first .. first + count - 1 alone (first a multiple of 4): Philox evaluated for exactly
    the groups first / 4 .. that hold them.  ``swap_offset_halves``: a deliberate mistake, counter words 2 and 3 exchanged."""
    assert first % 4 == 0
    groups = (count + 3) // 4
    g = np.uint64(first // 4) + np.arange(groups, dtype=np.uint64)
    lo, hi = offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF
    if swap_offset_halves:
        lo, hi = hi, lo
    counter = np.stack([g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), np.full(groups, lo, dtype=np.uint64),
                        np.full(groups, hi, dtype=np.uint64)], axis=-1)
    words = O.philox4x32_10(counter, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(-1)[:count]
    return words.astype(np.uint64) < np.uint64(philox_threshold(keep_prob))
