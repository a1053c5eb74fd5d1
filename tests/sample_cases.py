"""TEST INFRASTRUCTURE ONLY -- the fixed case lists of the sampling tests and the harness that calls npm_sample_rows through the C
ABI.  tests/test_sample_host.py checks, on tests/sample_reference.py alone, the properties of these lists that
tests/test_gpu_sample.py relies on, so that no case is ever skipped on the GPU."""

import ctypes as C
import itertools

import numpy as np

import sample_reference as SR

LDS_ROW = 32768                                   # include/npm_hip.h NPM_SAMPLE_LDS_ROW: the longest row the kernel keeps in LDS
C_LOGIT, LOW_LOGIT = np.float32(1.5), np.float32(-200.0)

# ---- (a) exact rows --------------------------------------------------------------------------------------------------------------------
EXACT_VOCABS = [1, 2, 63, 64, 65, 255, 1000, 4099, LDS_ROW - 1, LDS_ROW, LDS_ROW + 1, 65537]
EXACT_DRAWS = 16


def exact_params(vocab: int):
    """(temperature, top_k, top_p): greedy, then t x top-k x top-p."""
    grid = itertools.product([0.5, 1.0, 3.0], [0, 1, 2, 5, vocab, vocab + 7], [1.0, 0.5, 0.25, 1e-6])
    return [(0.0, 0, 1.0)] + list(grid)


def exact_rows(vocab: int) -> np.ndarray:
    """Four rows over {c, -200, -inf}: a mix; mostly c with ties everywhere; ONE c among -200 (a single candidate that top-k
    2 and 5 surround with tokens that can never be drawn); a few c among many -inf with -200 between.  Every row holds a c, except
    the last at vocab 1 (its only logit is -200: the maximum, weight 2^32)."""
    rng = np.random.default_rng(1000 + vocab)
    values = np.array([C_LOGIT, LOW_LOGIT, -np.inf], dtype=np.float32)
    rows = np.stack([values[rng.choice(3, size=vocab, p=probs)] for probs in
                     ([0.3, 0.5, 0.2], [0.9, 0.08, 0.02], [0.0, 1.0, 0.0], [0.02, 0.18, 0.8])])
    for r, at in enumerate(rng.integers(0, vocab, size=4)):
        rows[r, at] = C_LOGIT
    if vocab == 1:
        rows[3, 0] = LOW_LOGIT
    return rows


EXACT_SEEDS = [0, 1, 0x9E3779B97F4A7C15, 2 ** 64 - 1]

# ---- (d) general rows ------------------------------------------------------------------------------------------------------------------
GENERAL_VOCABS = [1000, 8195]
GENERAL_FAMILIES = [(0.7, 0, 1.0), (0.7, 50, 1.0), (0.7, 0, 0.9), (0.7, 50, 0.9), (1.3, 50, 1.0)]     # (t, top_k, top_p)
GENERAL_DRAWS, GENERAL_BATCH = 64, 4
GENERAL_SEEDS = [11, 12, 13, 14]
EPS = 2e-5            # admissible mass error, relative to the row's mass: derivation in tests/test_gpu_sample.py


def general_rows(vocab: int) -> np.ndarray:
    return (4 * np.random.default_rng(2000 + vocab).standard_normal([GENERAL_BATCH, vocab])).astype(np.float32)


# ---- the harness -----------------------------------------------------------------------------------------------------------------------
GUARD = 8                                          # sentinel words around every output vector
SENTINEL32, SENTINEL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


class Call:
    """One logit matrix on the device with its parameter vectors; ``step()`` launches npm_sample_rows once and returns
    (token, kept, prob, draw) as host arrays, after checking that the guard words around all four kept their sentinels.

    ``pitch`` (>= V): the columns behind V hold +inf and NaN alternately.  ``offset``: floats in front of the matrix (1: a base 4
    bytes off 16-byte alignment)."""

    def __init__(self, npm, logits, temperature, top_k, top_p, seed, draw=None, active=None, pitch=None, offset=0):
        from np_modeling_amd import _C, device as D
        self._C, self._D = _C, D
        logits = np.asarray(logits, dtype=np.float32)
        self.batch, self.vocab = logits.shape
        b = self.batch
        self.pitch = self.vocab if pitch is None else pitch
        host = np.empty([offset + b * self.pitch], dtype=np.float32)
        host[:offset] = np.nan
        padded = host[offset:].reshape(b, self.pitch)
        padded[:, self.vocab:] = np.where(np.arange(self.pitch - self.vocab) % 2 == 0, np.float32(np.inf), np.float32(np.nan))
        padded[:, :self.vocab] = logits
        self.logits = D.from_host(host)
        self.set_params(temperature, top_k, top_p, seed, draw, active)

    def set_params(self, temperature, top_k, top_p, seed, draw=None, active=None) -> 'Call':
        """New parameter vectors, counters and (sentinel-filled) outputs for the same logits on the device."""
        D, b = self._D, self.batch
        vec = lambda v, dtype: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), [b]))
        params = np.concatenate([vec(seed, np.uint64).view(np.uint8), vec(temperature, np.float32).view(np.uint8),
                                 vec(top_k, np.int32).view(np.uint8), vec(top_p, np.float32).view(np.uint8)])
        self.params = D.bytes_from_host(params)
        self.active = None if active is None else D.bytes_from_host(np.asarray(active, dtype=np.int32))
        draws = np.full([b + 2 * GUARD], SENTINEL64, dtype=np.uint64)
        draws[GUARD:GUARD + b] = vec(0 if draw is None else draw, np.uint64)
        self.draws = D.bytes_from_host(draws)
        self.out = D.bytes_from_host(np.full([3 * b + 4 * GUARD], SENTINEL32, dtype=np.uint32))
        return self

    def step(self):
        b, p = self.batch, self.params.ptr
        at = lambda j: self.out.ptr + 4 * (GUARD + j * (b + GUARD))
        desc = self._C.npm_sample(logits=self.logits.ptr + 4 * (self.logits.size - b * self.pitch), pitch=self.pitch, batch=b,
                                  vocab=self.vocab, temperature=p + 8 * b, top_k=p + 12 * b, top_p=p + 16 * b, seed=p,
                                  draw=self.draws.ptr + 8 * GUARD, active=None if self.active is None else self.active.ptr,
                                  token=at(0), kept=at(1), prob=at(2))
        self._C.check(self._C.lib().npm_sample_rows(C.byref(desc)), 'npm_sample_rows')
        out = self.out.numpy().view(np.uint32)
        draws = self.draws.numpy().view(np.uint64)
        cut = lambda j: out[GUARD + j * (b + GUARD):GUARD + j * (b + GUARD) + b]
        guards = np.concatenate([out[:GUARD]] + [out[GUARD + j * (b + GUARD) + b:GUARD + (j + 1) * (b + GUARD)] for j in range(3)])
        assert (guards == SENTINEL32).all(), 'a guard word around token / kept / prob was written'
        assert (draws[:GUARD] == SENTINEL64).all() and (draws[GUARD + b:] == SENTINEL64).all(), 'a guard word around draw was written'
        return cut(0).view(np.int32).copy(), cut(1).view(np.int32).copy(), cut(2).view(np.float32).copy(), draws[GUARD:GUARD + b].copy()


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
