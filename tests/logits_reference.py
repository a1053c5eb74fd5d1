"""TEST INFRASTRUCTURE ONLY -- the contracts of npm_logits_process, npm_history_append and npm_logprob_rows (include/npm_hip.h)
restated in NumPy float32 scalars and plain Python loops, and the fp64 log-softmax model general rows are judged against.

npm_logits_process, per active slot b and row r in 0 .. n_b:
  S_r = history[b, :L_b] + draft[b, :r]; ids outside 0 .. V - 1 are ignored; seen_i: i occurs in S_r; c_i: its occurrences at
  positions >= P_b; gen_r = (L_b - P_b) + r.
  1. seen_i and rep finite, > 0, != 1:            z_i = z_i / rep if z_i > 0 else z_i * rep
  2. c_i > 0 (unless freq == 0 and pres == 0):     z_i = z_i - freq * float32(c_i); z_i = z_i - pres
  3. the first bias entry per in-range index:      z_i = z_i + value
  4. 0 <= eos < V and gen_r < min_new:             z_eos = -inf
every operation a float32 operation of its own.  ``process`` also returns which elements a step applied to: everything else must
keep its bits, and a NaN a step produces is compared as a NaN (IEEE leaves its sign and payload open).

npm_logprob_rows is ``beam_reference.row_list`` with cum = 0 plus the chosen token's score by the same expression.
"""

import math

import numpy as np

import sample_reference as SR
from beam_reference import eps, model_lse, row_list          # noqa: F401  (re-exported: the tests take them from here)

F32 = np.float32
NAN32 = np.float32(np.nan)


def clip(v, lo, hi):
    return max(lo, min(int(v), hi))


def sequence(history_row, length, draft_row, r):
    """S_r as a list."""
    return [int(t) for t in history_row[:length]] + [int(t) for t in draft_row[:r]]


def process_row(z, seq, prompt, gen, rep, pres, freq, eos, min_new, bias, vocab):
    """One row, in place, from its S_r (``seq``) and the slot's parameters; ``bias``: the slot's (index, value) entries in list
    order; ``eos`` None: no rule.  Returns the set of token ids a step applied to."""
    rep, pres, freq = F32(rep), F32(pres), F32(freq)
    seen, count = set(), {}
    for pos, t in enumerate(seq):
        if 0 <= t < vocab:
            seen.add(t)
            if pos >= prompt:
                count[t] = count.get(t, 0) + 1
    rep_on = bool(np.isfinite(rep) and rep > 0 and rep != 1)
    pen_on = not (freq == 0 and pres == 0)
    first_bias = {}
    for index, value in bias:
        if 0 <= index < vocab and index not in first_bias:
            first_bias[int(index)] = F32(value)
    eos_on = eos is not None and 0 <= eos < vocab and gen < min_new
    written = set()
    with np.errstate(all='ignore'):
        for i in sorted(seen | set(first_bias)):
            v = F32(z[i])
            if rep_on and i in seen:
                v = F32(v / rep) if v > 0 else F32(v * rep)
                written.add(i)
            if pen_on and count.get(i, 0) > 0:
                f = F32(freq * F32(count[i]))
                v = F32(v - f)
                v = F32(v - pres)
                written.add(i)
            if i in first_bias:
                v = F32(v + first_bias[i])
                written.add(i)
            z[i] = v
    if eos_on:
        z[eos] = F32(-np.inf)
        written.add(int(eos))
    return written


def process(z, batch, rows, vocab, history=None, history_len=None, history_cap=0, prompt_len=None, draft=None, n_draft=None,
            active=None, repetition=None, presence=None, frequency=None, eos=None, min_new=None, bias_index=None, bias_value=None,
            bias_count=None, bias_cap=0):
    """The whole call on ``z`` [batch * rows, >= vocab] float32, IN PLACE (only the first ``vocab`` columns are ever touched);
    None stands for a NULL pointer.  Returns the boolean array of the elements a step applied to."""
    written = np.zeros(z.shape, dtype=bool)
    for b in range(batch):
        if active is not None and active[b] == 0:
            continue
        n = 0
        if n_draft is not None:
            if n_draft[b] < 0:
                continue
            n = min(int(n_draft[b]), rows - 1)
        length = clip(history_len[b], 0, history_cap) if history is not None else 0
        prompt = clip(prompt_len[b], 0, length) if prompt_len is not None else 0
        entries = []
        if bias_cap > 0:
            k = clip(bias_count[b], 0, bias_cap)
            entries = [(int(bias_index[b][j]), bias_value[b][j]) for j in range(k)]
        for r in range(n + 1):
            seq = sequence(history[b] if history is not None else [], length, draft[b] if draft is not None else [], r)
            done = process_row(z[b * rows + r], seq, prompt, length - prompt + r,
                               1.0 if repetition is None else repetition[b], 0.0 if presence is None else presence[b],
                               0.0 if frequency is None else frequency[b],
                               None if eos is None or min_new is None else int(eos[b]), 0 if min_new is None else int(min_new[b]),
                               entries, vocab)
            written[b * rows + r, sorted(done)] = True
    return written


def same(got, want, written) -> bool:
    """Bit for bit, except that where a step applied and the reference has a NaN any NaN will do."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    equal = got.view(np.uint32) == want.view(np.uint32)
    return bool((equal | (written & np.isnan(got) & np.isnan(want))).all())


def history_append(history, lengths, cap, ids, active=None):
    """npm_history_append on host arrays, in place."""
    for b in range(len(lengths)):
        if active is not None and active[b] == 0:
            continue
        if ids[b] < 0:
            continue
        at = max(int(lengths[b]), 0)
        if at < cap:
            history[b][at] = ids[b]
            lengths[b] = at + 1


def logprob_row(z, token, top_n, weights=SR.weights32):
    """(lse, chosen, top tokens [top_n], top log-probabilities [top_n]) of one row; ``token`` None: no ids (chosen NaN)."""
    z = np.asarray(z, dtype=np.float32)
    tokens, scores = np.full([top_n], -1, dtype=np.int32), np.full([top_n], -np.inf, dtype=np.float32)
    if (token is not None and token < 0) or SR.invalid_row(z, 1.0, 1.0):
        return NAN32, NAN32, tokens, scores
    count, toks, vals, lse = row_list(z, np.float32(0), top_n, weights)
    tokens[:count], scores[:count] = toks, vals
    chosen = NAN32
    if token is not None and token < z.size:
        zmax = np.float64(z.max() + np.float32(0))
        w = np.asarray(weights(z, 1.0))
        n = math.log(float(sum(int(v) for v in w[z > -np.inf])) * 2.0 ** -32)
        with np.errstate(invalid='ignore'):
            chosen = np.float32(((np.float64(np.float32(0)) - zmax) - n) + np.float64(z[token]))
    return lse, chosen, tokens, scores


def model_logprobs(z):
    """fp64 log-softmax of one valid row; -inf at masked tokens."""
    z64 = np.asarray(z, dtype=np.float32).astype(np.float64)
    return z64 - model_lse(z)
