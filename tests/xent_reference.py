"""TEST INFRASTRUCTURE ONLY -- softmax cross-entropy from logits and token ids, restated in float64, with the rules and the error
bound that include/npm_hip.h states for npm_softmax_xent_rows.  tests/hostsim/training.py answers the entry point with it on the host;
tests/test_gpu_xent.py holds the kernel to it."""

from collections import namedtuple

import numpy as np

U = 2.0 ** -24

Result = namedtuple('Result', 'row_loss lse grad loss_sum')


def as_e(smoothing):
    """The smoothing the kernel sees: a float32."""
    return float(np.float32(smoothing))


def log_sum_exp(z):
    """float64 log-sum-exp of one row with a finite maximum; -inf entries add nothing."""
    m = z.max()
    return m + np.log(np.exp(z - m).sum())


def reference(logits, targets, smoothing=0.0, grad_scale=1.0, need_grad=True):
    """logits [R, V] (any float dtype; read as float64), targets [R] integers -> Result of float64 arrays (grad None without)."""
    z = np.asarray(logits, dtype=np.float64)
    t = np.asarray(targets).astype(np.int64)
    rows, vocab = z.shape
    e, gs = as_e(smoothing), float(np.float32(grad_scale))
    row_loss, lse = np.zeros(rows), np.full(rows, np.nan)
    grad = np.zeros((rows, vocab)) if need_grad else None
    with np.errstate(all='ignore'):
        for r in range(rows):
            if t[r] < 0:                                            # ignored: zeros, the row is not read
                continue
            row = z[r]
            invalid = np.isnan(row).any() or np.isposinf(row).any() or np.isneginf(row).all()
            if t[r] >= vocab or invalid:
                row_loss[r] = np.nan
                if need_grad:
                    grad[r] = np.nan
                continue
            lse[r] = log_sum_exp(row)
            logp = row - lse[r]
            row_loss[r] = -(1.0 - e) * logp[t[r]]
            if e != 0.0:
                row_loss[r] -= e / vocab * logp.sum()
            if need_grad:
                p = np.exp(logp)
                g = p - e / vocab
                p[t[r]] = 0.0                                       # 1 - p_t as the sum of the others: no cancellation near p_t = 1
                g[t[r]] = e * (1.0 - 1.0 / vocab) - p.sum()
                g[np.isneginf(row)] = 0.0                           # a masked token, the target included
                grad[r] = gs * g
    return Result(row_loss, lse, grad, row_loss.sum())


def bounds(logits, targets, smoothing=0.0, grad_scale=1.0):
    """(bound of row_loss [R], of lse [R], of grad [R, V]) as include/npm_hip.h derives them; only meaningful where the reference
    is finite.  A -inf logit has d_j = inf and p_j = 0: its terms are 0."""
    z = np.asarray(logits, dtype=np.float64)
    t = np.asarray(targets).astype(np.int64)
    rows, vocab = z.shape
    e, gs = as_e(smoothing), abs(float(np.float32(grad_scale)))
    ref = reference(z, t, smoothing, grad_scale)
    gamma = (55 + vocab / 1024) * 2.0 ** -53
    b_loss, b_lse, b_grad = np.zeros(rows), np.zeros(rows), np.zeros((rows, vocab))
    with np.errstate(all='ignore'):
        for r in range(rows):
            if t[r] < 0 or t[r] >= vocab or not np.isfinite(ref.lse[r]):
                continue
            row = z[r]
            m = row.max()
            p = np.exp(row - ref.lse[r])
            d = np.where(p > 0, m - row, 0.0)
            a = float((p * d).sum())
            finite = row[np.isfinite(row)]
            b_lse[r] = U * (abs(ref.lse[r]) + 1.01 * (a + 2)) + gamma * (1 + abs(m))
            if np.isfinite(ref.row_loss[r]):
                b_loss[r] = U * (abs(ref.row_loss[r]) + 1.01 * (a + 2)) + gamma * (1 + abs(m) + abs(row[t[r]]) + e * np.abs(finite).mean())
            q = p * (d + 1.01 * a + 6.1)
            pt = p[t[r]]
            rest = float(np.delete(p, t[r]).sum())                  # 1 - p_t without cancellation
            q[t[r]] = (a - pt * d[t[r]]) + 2 * rest + 1.01 * rest * (a + 2)
            g_over = np.abs(ref.grad[r]) / gs if gs else np.zeros(vocab)
            b_grad[r] = 1.01 * U * gs * (q + e / vocab + 2 * g_over) + 2.0 ** -125 * gs
    return b_loss, b_lse, b_grad


def worst_fraction(got, want, bound):
    """max |got - want| / bound over the finite entries of ``want``; asserts first that got and want agree on where they are NaN,
    +inf and -inf, and that no finite entry has a zero bound with a non-zero error."""
    got, want, bound = (np.asarray(x, dtype=np.float64) for x in (got, want, bound))
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    finite = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN pattern'
    assert np.array_equal(got[~finite & ~np.isnan(want)], want[~finite & ~np.isnan(want)]), 'inf pattern'
    err = np.abs(got[finite] - want[finite])
    assert np.isfinite(err).all(), 'a finite reference entry came out non-finite'
    lim = bound[finite]
    assert not ((lim == 0) & (err != 0)).any(), 'an entry that must be exact is not'
    frac = np.divide(err, lim, out=np.zeros_like(err), where=lim > 0)
    return float(frac.max()) if frac.size else 0.0
