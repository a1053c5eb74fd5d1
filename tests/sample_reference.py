"""TEST INFRASTRUCTURE ONLY -- the contract of npm_sample_rows (include/npm_hip.h) restated in NumPy and Python integers.

One row, with z its fp32 logits:
 1. A row that holds a NaN or +inf, or whose every logit is -inf, is invalid (so is a temperature that is not >= 0 and a top_p
    that is not > 0): token -1, kept 0, prob 0.  -inf logits are otherwise legal and never kept.
 2. Order: i before j when z_i > z_j, or z_i == z_j and i < j; -0.0 == 0.0.
 3. Greedy (temperature == 0 or top_k == 1): the first token in order, kept 1, prob 1.
 4. K1: the first min(top_k, finite count) tokens in order; top_k <= 0: every finite token.
 5. w_i = floor(q_i 2^32) as an integer, q_i = exp((z_i - zmax) * (1 / t)) in fp32.  Every mass is an integer sum of w.
 6. K2: the shortest prefix of K1 in order whose mass reaches max(1, floor(double(top_p) * double(W1))); top_p >= 1: K1.
 7. u24 = word0 >> 8 of Philox4x32-10(counter (draw lo, draw hi, 0, 0), key (seed lo, seed hi)); target = floor(Wk u24 / 2^24);
    the token is the first i of K2 IN INDEX ORDER whose running mass exceeds target; prob = float32(double(w) / double(Wk)).
 8. draw += 1 for every active row; an inactive row: token -1, kept 0, prob 0, draw unchanged, nothing read.

``sample_exact`` is this, given integer weights: the model the kernel must EQUAL on rows whose weights are exact
(``exact_weights``: every fp32 exponent argument is 0 or below -60, so w is 2^32 or 0 whatever the exponential's last bit).
``Float64Row`` is the fp64 model of the same steps for general rows: which ``kept`` and which tokens are admissible within a
relative mass error ``eps``.
"""

import functools

import numpy as np

from oracle.np_oracle import philox4x32_10

ONE = 1 << 32


@functools.lru_cache(maxsize=None)
def u24_of(seed: int, draw: int) -> int:
    counter = np.array([draw & 0xFFFFFFFF, (draw >> 32) & 0xFFFFFFFF, 0, 0], dtype=np.uint64)
    return int(philox4x32_10(counter, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[0]) >> 8


def invalid_row(z, t, p) -> bool:
    z = np.asarray(z, dtype=np.float32)
    return bool(np.isnan(z).any() or (z == np.inf).any() or not (z > -np.inf).any() or not t >= 0 or not np.float32(p) > 0)


def order_of(z) -> np.ndarray:
    """Token indices in the order of step 2."""
    z = np.asarray(z, dtype=np.float32)
    return np.argsort(-(z + np.float32(0)), kind='stable')          # x + 0 turns -0.0 into 0.0; stable: ties by index


def exponent_args(z, t) -> np.ndarray:
    """(z - zmax) * (1 / t) as the kernel forms it: three fp32 roundings."""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        return (z - z.max()) * (np.float32(1) / np.float32(t))


def exact_weights(z, t) -> np.ndarray:
    """int64 weights of a row whose weights do not depend on the exponential's rounding: every argument is 0 (w = 2^32) or
    below -60 (exp < 2^-86, w = 0).  AssertionError for any other row."""
    a = exponent_args(z, t)
    assert ((a == 0) | (a < -60)).all(), 'not an exact row'
    return np.where(a == 0, ONE, 0).astype(np.int64)


def weights32(z, t) -> np.ndarray:
    """Step 5 with NumPy's float32 exponential (the host simulator's weights; not bit for bit the device's)."""
    with np.errstate(over='ignore', under='ignore'):
        q = np.exp(exponent_args(z, t).astype(np.float32))
    return np.floor(q.astype(np.float64) * 4294967296.0).astype(np.int64)


class ExactRow:
    """Steps 1-6 of one (row, parameters) with integer weights ``w`` (None for a greedy or invalid row); ``draw(seed, counter)``
    is step 7: (token, kept, prob)."""

    def __init__(self, z, t, k, p, w=None, order=None):
        z = np.asarray(z, dtype=np.float32)
        self.invalid = invalid_row(z, t, p)
        self.greedy = not self.invalid and (t == 0 or k == 1)
        if self.invalid:
            return
        order = order_of(z) if order is None else order                # a caller with many parameter sets sorts once
        self.first = int(order[0])
        if self.greedy:
            return
        w = exact_weights(z, t) if w is None else np.asarray(w, dtype=np.int64)
        finite = int((z > -np.inf).sum())
        k1 = order[:finite if k <= 0 else min(int(k), finite)]
        cum = np.cumsum(w[k1])
        n = k1.size
        if np.float32(p) < 1:
            need = max(1, int(np.floor(np.float64(np.float32(p)) * np.float64(int(cum[-1])))))
            n = int(np.searchsorted(cum, need, side='left')) + 1
        self.kept = n
        self.k2 = np.sort(k1[:n])                                  # index order
        self.w = w
        self.running = np.cumsum(w[self.k2])
        self.mass = int(self.running[-1])

    def draw(self, seed: int, counter: int):
        if self.invalid:
            return -1, 0, np.float32(0)
        if self.greedy:
            return self.first, 1, np.float32(1)
        target = (self.mass * u24_of(seed, counter)) >> 24
        token = int(self.k2[np.searchsorted(self.running, target, side='right')])
        return token, self.kept, np.float32(np.float64(int(self.w[token])) / np.float64(self.mass))


def sample_exact(z, t, k, p, seed, counter, w=None):
    """(token, kept, prob, counter + 1) of one active row."""
    return ExactRow(z, t, k, p, w).draw(seed, counter) + (counter + 1,)


class Float64Row:
    """The fp64 model of one general (row, parameters): t > 0, top_k != 1, a valid row.  ``kept_set(eps)``: every admissible
    ``kept``; ``token_set(n, u, eps)``: every admissible token given ``kept = n`` and the uniform u = u24 / 2^24."""

    def __init__(self, z, t, k, p):
        z64 = np.asarray(z, dtype=np.float32).astype(np.float64)
        self.p = float(np.float32(p))
        self.order = order_of(z)
        finite = int((z64 > -np.inf).sum())
        self.k1 = self.order[:finite if k <= 0 else min(int(k), finite)]
        self.q = np.exp((z64 - z64.max()) / float(np.float32(t)))
        self.c = np.cumsum(self.q[self.k1])                        # c[n - 1]: the mass of the first n tokens in order
        self.r1 = float(self.c[-1])
        self._running = {}

    def kept_set(self, eps: float):
        n1 = self.k1.size
        if self.p >= 1:
            return [n1]
        before = np.concatenate([[0.0], self.c[:-1]])              # c_{n-1}
        n = np.arange(1, n1 + 1)
        ok = ((self.c >= (self.p - eps) * self.r1) | (n == n1)) & (before < (self.p + eps) * self.r1)
        return n[ok].tolist()

    def _index_order(self, n: int):
        if n not in self._running:
            k2 = np.sort(self.k1[:n])
            self._running[n] = (k2, np.cumsum(self.q[k2]))
        return self._running[n]

    def token_set(self, n: int, u: float, eps: float):
        k2, s = self._index_order(n)
        rk = float(s[-1])
        before = np.concatenate([[0.0], s[:-1]])
        return k2[(before <= (u + eps) * rk) & (s > (u - eps) * rk)].tolist()

    def prob(self, n: int, token: int) -> float:
        return float(self.q[token] / self._index_order(n)[1][-1])
