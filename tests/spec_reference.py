"""TEST INFRASTRUCTURE ONLY -- the contracts of npm_ngram_draft and npm_verify_rows (include/npm_hip.h) restated as plain loops over
Python integers, the second on tests/sample_reference.py's ``ExactRow``.

``draft``: prompt lookup.  n walks from nmax down to nmin (an n with L < n + 1 is skipped); the candidates of n are the starts j in
0 .. L - n - 1 of an earlier occurrence of the last n tokens; the first n with a candidate is used, among its candidates the
LARGEST j with j + n + m_max <= L, else the SMALLEST; m = min(m_max, L - (j + n)), m_max = min(T, limit).

``verify``: row r of a slot is sampled at counter draw + r (mod 2^64); a = the first r in 0 .. n that is n, or whose sample is not
draft[r] (a draft below 0 never matches; an invalid row samples -1); tokens behind a are -1 with kept 0 and prob 0; the counter
advances by a + 1.
"""

import numpy as np

import sample_reference as SR


def draft(history, max_draft, limit, nmax, nmin):
    """(chunk of max_draft + 1 ints, n_new, (n, j, m)) for one slot; (n, j) None where nothing matched."""
    h, t = [int(v) for v in history], int(max_draft)
    length = len(h)
    if length == 0 or limit < 0:
        return [-1] * (t + 1), 0, (None, None, 0)
    m_max = min(t, int(limit))
    chosen = (None, None)
    if m_max > 0:
        for n in range(nmax, nmin - 1, -1):
            if length < n + 1:
                continue
            candidates = [j for j in range(length - n) if h[j:j + n] == h[length - n:]]
            if candidates:
                whole = [j for j in candidates if j + n + m_max <= length]
                chosen = (n, max(whole) if whole else min(candidates))
                break
    n, j = chosen
    m = 0 if j is None else min(m_max, length - (j + n))
    chunk = [h[-1]] + [h[j + n + i] for i in range(m)] + [-1] * (t - m)
    return chunk, 1 + m, (n, j, m)


def verify(z, t, k, p, seed, counter, drafted, n, weights=None):
    """One slot: ``z`` [rows, V] logits, ``drafted`` its draft, ``n`` how many of it count (below 0: inactive).
    (tokens [rows], accepted, counter after, kept [rows], prob [rows]).  ``weights(z_row, t)``: the integer weights of a general
    row (default: the row must be exact, ``SR.exact_weights``)."""
    z = np.asarray(z, dtype=np.float32)
    rows = z.shape[0]
    tokens, kept, prob = [-1] * rows, [0] * rows, [np.float32(0)] * rows
    if n < 0:
        return tokens, 0, counter, kept, prob
    a = n
    for r in range(n + 1):
        general = t > 0 and k != 1 and not SR.invalid_row(z[r], t, p)
        row = SR.ExactRow(z[r], float(t), int(k), float(p), weights(z[r], t) if general and weights is not None else None)
        tokens[r], kept[r], prob[r] = row.draw(int(seed), (int(counter) + r) % (1 << 64))
        if r < n and (int(drafted[r]) < 0 or tokens[r] != int(drafted[r])):
            a = r
            break
    return tokens, a, (int(counter) + a + 1) % (1 << 64), kept, prob
