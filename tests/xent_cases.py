"""TEST INFRASTRUCTURE ONLY -- the shapes and the data the softmax cross-entropy tests share.

INSTANCES is the one table of the kernel's instance boundaries (np_modeling_amd/csrc/npm_xent.hip picks by vocabulary alone); the
vocabularies of the cases are generated from it: every boundary, one below it and one above it, plus the fixed list."""

from collections import namedtuple

import numpy as np

# (name npm_last_xent_kernel reports, smallest V, largest V or None)
INSTANCES = (
    ('xent_wave', 1, 1024),
    ('xent_block256', 1025, 8192),
    ('xent_block1024', 8193, 32768),
    ('xent_block1024_global', 32769, None),
)
LDS_ROW = 32768                                     # the largest row that is read once (the sampler's LDS row, NPM_SAMPLE_LDS_ROW)
FIXED_VOCABS = (1, 2, 3, 63, 64, 65, 255, 257, 1000, LDS_ROW, LDS_ROW + 1, 40003)
ROWS = (1, 2, 5, 64)
SCALES = (1.0, 10.0, 80.0)                          # at 80 all but a few exp underflow
IGNORE = ('none', 'first', 'last', 'all')


def instance_of(vocab):
    return next(name for name, low, high in INSTANCES if vocab >= low and (high is None or vocab <= high))


def vocabs():
    out = set(FIXED_VOCABS)
    for _, low, high in INSTANCES:
        for edge in (low, high):
            if edge is not None:
                out.update(v for v in (edge - 1, edge, edge + 1) if v >= 1)
    return sorted(out)


# pad: pitch - V (0 tight, 1 unaligned: the scalar path whenever rows > 1, 4 covering); offset: floats between the 16-byte aligned
# allocation and the first logit (1: an unaligned base, the scalar path)
Case = namedtuple('Case', 'index vocab rows pad offset scale smoothing ignore')


def _cases():
    out = []
    for i, vocab in enumerate(vocabs()):
        for k, pad in enumerate((0, 1, 4)):
            n = len(out)                        # strides coprime to the list lengths: the properties do not move in step
            out.append(Case(n, vocab, ROWS[(i + k) % 4], pad, 1 if n % 5 == 2 else 0, SCALES[n % 3], (0.0, 0.1)[(n // 2) % 2],
                            IGNORE[(i + 2 * k) % 4]))
    return out


CASES = _cases()


def case_id(case):
    return 'V%d-R%d-pad%d-off%d-s%g-e%g-%s' % case[1:]


def data(case):
    """(logits [rows, V] float32, targets [rows] int32) of a case.  Row r: r % 5 == 0 has its target at 0, r % 5 == 1 at V - 1,
    r % 5 == 2 is a row of equal logits, r % 5 == 3 carries a block of -inf over the middle third (the target outside it); the
    ignore pattern sets targets to -1."""
    rng = np.random.default_rng(1000 + case.index)
    v, rows = case.vocab, case.rows
    z = (case.scale * rng.standard_normal((rows, v))).astype(np.float32)
    t = rng.integers(0, v, size=rows).astype(np.int32)
    for r in range(rows):
        if r % 5 == 0:
            t[r] = 0
        elif r % 5 == 1:
            t[r] = v - 1
        elif r % 5 == 2:
            z[r] = np.float32(0.37 * case.scale)
        elif r % 5 == 3 and v >= 3:
            z[r, v // 3:2 * v // 3] = -np.inf
            t[r] = 0
    if case.ignore == 'first':
        t[0] = -1
    elif case.ignore == 'last':
        t[-1] = -1
    elif case.ignore == 'all':
        t[:] = -1
    return z, t
