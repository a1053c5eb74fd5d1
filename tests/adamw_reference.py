"""TEST INFRASTRUCTURE ONLY -- NumPy models of npm_sumsq_ranges, npm_clip_finish and npm_adamw_step (include/npm_hip.h), each
operation in the precision the header states, and the bounds the tests hold them to.  Nothing here is measured.

* the sum of squares: ``math.fsum`` over the exact fp64 squares (a product of two float32 is exact in fp64; fsum rounds the exact
  sum once).  Bound: |got - exact| <= N 2^-53 exact with N the number of elements.  Every term is >= 0, so every partial sum of
  ANY order of fp64 additions is at most the total; each of the at most N additions errs by at most 2^-53 of its own result.
* the clip factor: the header's expression, evaluated by NumPy in fp64 and rounded once to float32: bit for bit.
* the step: moments bit for bit; the parameter bit for bit except at near ties of its ONE final rounding (``near_tie`` of
  tests/optim_reference.py, the rule Adam is held to), where one float32 ulp is allowed; at most ``MAX_EXEMPT`` such elements a
  case, counted from the model alone."""

import math
from typing import NamedTuple, Optional

import numpy as np

import optim_reference as R

TILE = 16384
HYPER = (1e-3, 0.9, 0.999, 1e-8)                     # lr, beta1, beta2, epsilon: the class's defaults at lr 1e-3
MAX_EXEMPT = R.MAX_EXEMPT


def exact_sumsq(*arrays) -> float:
    terms = []
    for a in arrays:
        x = np.asarray(a, dtype=np.float32).astype(np.float64).ravel()
        terms += (x * x).tolist()
    return math.fsum(terms)


def sumsq_bound(count: int, exact: float) -> float:
    return count * 2.0 ** -53 * exact


def sumsq_check(got: float, arrays, what='') -> float:
    """Asserts the bound; returns the error as a fraction of it (0 where the bound is 0)."""
    exact, count = exact_sumsq(*arrays), sum(np.asarray(a).size for a in arrays)
    err, bound = abs(got - exact), sumsq_bound(count, exact)
    assert err <= bound, f'{what}: |{got!r} - {exact!r}| = {err:.3e} > {bound:.3e} (N = {count})'
    return err / bound if bound else 0.0


def clip_finish(sumsq: float, max_norm: float):
    """(norm, scale, ok) as doubles."""
    with np.errstate(all='ignore'):
        norm = np.sqrt(np.float64(sumsq))
        if not np.isfinite(norm):
            return float(norm), 0.0, 0.0
        ratio = np.float64(max_norm) / (norm + np.float64(1e-6))
        return float(norm), float(np.float32(min(np.float64(1.0), ratio))), 1.0


class AdamWStep(NamedTuple):
    p: np.ndarray         # float32 parameter after the step
    m: np.ndarray         # float64 first moment after it
    v: np.ndarray         # float64 second moment
    d: np.ndarray         # the float64 value p is the rounding of
    upd: np.ndarray       # the float64 step


def adamw_model(p, g, m, v, step: int, hyper=HYPER, weight_decay: float = 0.0, clip: Optional[tuple] = None,
                variant=None) -> AdamWStep:
    """One step.  ``clip`` = None (clip_state NULL) or (scale, ok).  ``variant`` names one deliberate mistake: 'eps_inside' (Adam's
    root), 'f32_products' (Adam's float32 gradient products), 'coupled' (the decay added to the gradient: Adam with L2)."""
    lr, b1, b2, eps = (float(h) for h in hyper)
    p, g = np.asarray(p, dtype=np.float32), np.asarray(g, dtype=np.float32)
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if clip is not None and clip[1] == 0:
        zero = np.zeros(p.shape)
        return AdamWStep(p.copy(), m.copy(), v.copy(), p.astype(np.float64), zero)
    omb1, omb2, c1, c2, lw = 1.0 - b1, 1.0 - b2, 1.0 - b1 ** step, 1.0 - b2 ** step, lr * float(weight_decay)
    with np.errstate(all='ignore'):
        if clip is not None:
            g = np.float32(clip[0]) * g                                   # one float32 product
        G = g.astype(np.float64)
        if variant == 'coupled':
            G = G + weight_decay * p.astype(np.float64)
        if variant == 'f32_products':
            t1, t2 = (np.float32(omb1) * g).astype(np.float64), (np.float32(omb2) * (g * g)).astype(np.float64)
        else:
            t1, t2 = omb1 * G, omb2 * (G * G)
        nm, nv = b1 * m + t1, b2 * v + t2
        p64 = p.astype(np.float64)
        d = p64 if variant == 'coupled' else p64 - lw * p64
        if variant == 'eps_inside':
            upd = lr * ((nm / c1) / np.sqrt(nv / c2 + eps))
        else:
            upd = lr * ((nm / c1) / (np.sqrt(nv / c2) + eps))
        out = d - upd
        return AdamWStep(out.astype(np.float32), nm, nv, out, upd)


def adamw_check(got_p, got_m, got_v, want: AdamWStep, what='') -> tuple:
    """(near ties in the case, of those the number where the parameter differs); asserts everything in the module docstring."""
    assert np.array_equal(R.bits(got_m), R.bits(want.m)), f'{what}: first moment differs in {int((R.bits(got_m) != R.bits(want.m)).sum())} elements'
    assert np.array_equal(R.bits(got_v), R.bits(want.v)), f'{what}: second moment differs in {int((R.bits(got_v) != R.bits(want.v)).sum())} elements'
    near = R.near_tie(want.d, want.upd)
    exempt = int(near.sum())
    assert exempt <= MAX_EXEMPT, f'{what}: {exempt} near-tie elements, more than {MAX_EXEMPT}: choose another seed'
    got_p = np.asarray(got_p, dtype=np.float32)
    differs = R.bits(got_p) != R.bits(want.p)
    bad = differs & ~near
    assert not bad.any(), (f'{what}: parameter differs in {int(bad.sum())} of {bad.size} elements that are no near ties; first at '
                           f'{int(np.flatnonzero(bad)[0])}: got {got_p[bad][0]!r}, want {want.p[bad][0]!r}')
    if differs.any():
        assert np.abs(R.ordered(got_p[differs]) - R.ordered(want.p[differs])).max() <= 1, f'{what}: a near tie is off by more than one ulp'
    return exempt, int(differs.sum())
