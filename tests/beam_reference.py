"""TEST INFRASTRUCTURE ONLY -- the contract of npm_beam_step (include/npm_hip.h) restated in NumPy, fp64 and Python integers, the
fp64 model general rows are judged against, and a plain Python beam search.

Slots are G groups of W beams, slot g W + w; C = 2 W.  One call:
 1. A dead row (cum == -inf, or NaN) is not read and contributes nothing.
 2. A live row with a NaN or +inf, or all -inf, is invalid: contributes nothing.  -inf masks a token.
 3. Row order: larger logit first, ties by index, -0.0 == 0.0 (``sample_reference.order_of``).
 4. W1 = sum floor(expf(z_i - zmax) 2^32) over the finite tokens as a Python integer.
 5. n = log(float(W1) * 2^-32) in fp64; lse = float32(float64(zmax) + n), zmax + 0.
 6. s = float32(((float64(cum_w) - float64(zmax_w)) - n_w) + float64(z_i)).
 7. Candidates of a group: larger score, then smaller beam, then row order.
 8. cand_slot / cand_token / cand_score [G, C]: the first C; -1 / -1 / -inf behind the last.
 9. The split (``split``): an eos below position W is finished, at or above W ignored; the others are the next beams until W.
10. parent / ids / cum per slot of the next step, lse per row of this one (NaN: dead or invalid).

``step`` is this, given a function for the integer weights (``sample_reference.weights32`` for the host simulator,
``exact_weights`` for rows whose weights do not depend on the exponential's last bit).  ``model_scores`` is the fp64 model and
``eps`` the derived bound between the two.  ``PyBeamSearch`` is ``np_modeling_amd.beam.BeamSearch`` in plain Python over fp64
log-probabilities.
"""

import math

import numpy as np

import sample_reference as SR

NAN32 = np.float32(np.nan)


def eps(s, vocab):
    """The bound on |device score - fp64 model|: one fp32 rounding of z - zmax (|d| <= 88: 88 * 2^-24 = 5.2e-6), the
    exponential's ulps (< 3e-7) and the floors (V 2^-32) in the normaliser, then one fp32 rounding of the score."""
    return 6e-6 + vocab * 2.0 ** -32 + 2.0 ** -23 * np.abs(s)


def live(c) -> bool:
    return bool(c > -np.inf)                                   # False for -inf and for NaN


def exact_weights(z, t=1.0):
    return SR.exact_weights(z, t)


def row_list(z, c, cands, weights):
    """Steps 2 - 6 of one live row: (count, tokens, scores float32, lse float32); count 0 and lse NaN for an invalid row."""
    z = np.asarray(z, dtype=np.float32)
    if SR.invalid_row(z, 1.0, 1.0):
        return 0, [], [], NAN32
    zmax = np.float64(z.max() + np.float32(0))
    w = np.asarray(weights(z, 1.0))
    w1 = sum(int(v) for v in w[z > -np.inf])
    n = math.log(float(w1) * 2.0 ** -32)
    finite = int((z > -np.inf).sum())
    tokens = [int(i) for i in SR.order_of(z)[:min(cands, finite)]]
    scores = [np.float32(((np.float64(c) - zmax) - n) + np.float64(z[i])) for i in tokens]
    return len(tokens), tokens, scores, np.float32(zmax + n)


def split(cand_slot, cand_token, cand_score, first, width, eos):
    """Step 9 and 10 on one group's candidate list: (parent, ids, cum, finished positions)."""
    parent, ids, cum = [-1] * width, [-1] * width, [np.float32(-np.inf)] * width
    finished, placed = [], 0
    for p in range(len(cand_slot)):
        if cand_slot[p] < 0:
            break
        if eos >= 0 and cand_token[p] == eos:
            if p < width:
                finished.append(p)
        elif placed < width:
            parent[placed], ids[placed], cum[placed] = int(cand_slot[p]), int(cand_token[p]), np.float32(cand_score[p])
            placed += 1
    return parent, ids, cum, finished


def step(logits, cum, groups, width, eos, weights=SR.weights32):
    """The whole call.  ``logits`` [G W, V] float32 (dead rows are never touched), ``cum`` [G W] float32.  A dict of cand_slot,
    cand_token, cand_score [G, C], parent, ids, cum (the next step's), lse [G W] and finished (per group: positions)."""
    cands, n = 2 * width, groups * width
    out = dict(cand_slot=np.full([groups, cands], -1, dtype=np.int32), cand_token=np.full([groups, cands], -1, dtype=np.int32),
               cand_score=np.full([groups, cands], -np.inf, dtype=np.float32), parent=np.full([n], -1, dtype=np.int32),
               ids=np.full([n], -1, dtype=np.int32), cum=np.full([n], -np.inf, dtype=np.float32),
               lse=np.full([n], np.nan, dtype=np.float32), finished=[])
    for g in range(groups):
        entries = []
        for w in range(width):
            r = g * width + w
            if not live(cum[r]):
                continue
            count, tokens, scores, out['lse'][r] = row_list(logits[r], cum[r], cands, weights)
            entries += [(-float(scores[j]), w, j, tokens[j], scores[j]) for j in range(count)]
        entries.sort(key=lambda e: e[:3])
        for p, (_, w, _, token, score) in enumerate(entries[:cands]):
            out['cand_slot'][g, p], out['cand_token'][g, p], out['cand_score'][g, p] = g * width + w, token, score
        parent, ids, nxt, finished = split(out['cand_slot'][g], out['cand_token'][g], out['cand_score'][g], g * width, width, eos)
        out['parent'][g * width:(g + 1) * width], out['ids'][g * width:(g + 1) * width] = parent, ids
        out['cum'][g * width:(g + 1) * width] = nxt
        out['finished'].append(finished)
    return out


def model_lse(z):
    """fp64 log-sum-exp of one valid row."""
    z64 = np.asarray(z, dtype=np.float32).astype(np.float64)
    zmax = z64.max()
    with np.errstate(under='ignore'):
        return zmax + np.log(np.exp(z64 - zmax).sum())


def model_scores(logits, cum):
    """fp64 [rows, V]: cum + log-softmax; -inf everywhere in a dead or invalid row (and at masked tokens)."""
    logits = np.asarray(logits, dtype=np.float32)
    out = np.full(logits.shape, -np.inf, dtype=np.float64)
    for r in range(logits.shape[0]):
        if live(cum[r]) and not SR.invalid_row(logits[r], 1.0, 1.0):
            out[r] = np.float64(cum[r]) + logits[r].astype(np.float64) - model_lse(logits[r])
    return out


def model_top(s, groups, width, count):
    """Per group: the first ``count`` candidates [(score, slot, token)] of the fp64 scores ``s`` (``model_scores``) under step
    7's order."""
    out = []
    for g in range(groups):
        block = s[g * width:(g + 1) * width]
        vocab = block.shape[1]
        flat = block.ravel()
        keep = min(flat.size, count + 2 * width * 2)
        near = np.argpartition(-flat, keep - 1)[:keep] if keep < flat.size else np.arange(flat.size)
        # ties by beam, then row order (which for equal logits is the index): the flat index is (beam, index)
        near = sorted(near.tolist(), key=lambda f: (-flat[f], f))
        out.append([(float(flat[f]), g * width + f // vocab, f % vocab) for f in near if flat[f] > -np.inf][:count])
    return out


class PyBeamSearch:
    """``np_modeling_amd.beam.BeamSearch`` in plain Python: ``search(logits)`` takes host logits [G W, V], works in fp64
    log-probabilities and returns (parents, ids, done).  ``gaps`` collects the differences between scores whose order decided
    something: neighbours among the candidates a step used -- the finished ones and the next beams -- down to the first
    candidate it did not use, and hypothesis scores compared when one is kept, dropped or decides that the group is done."""

    def __init__(self, groups, width, eos=None, length_penalty=1.0, max_new_tokens=None, early_stopping=True):
        self.groups, self.width, self.eos = groups, width, eos
        self.length_penalty, self.max_new_tokens, self.early_stopping = length_penalty, max_new_tokens, early_stopping
        self.cum = np.full([groups * width], -np.inf)
        self.cum[::width] = 0
        self.tokens = [[[]] + [None] * (width - 1) for _ in range(groups)]
        self.hyps = [[] for _ in range(groups)]
        self.steps = [0] * groups
        self.done = [False] * groups
        self.gaps, self.scores_seen = [], []

    def _keep(self, g, score, tokens):
        self.gaps += [abs(score - s) for s, _ in self.hyps[g]]
        self.hyps[g].append((score, tokens))
        self.hyps[g].sort(key=lambda h: -h[0])
        del self.hyps[g][self.width:]

    def hypotheses(self, g):
        return [(list(tokens), score) for score, tokens in self.hyps[g]]

    def search(self, logits):
        width, cands = self.width, 2 * self.width
        top = model_top(model_scores(logits, self.cum), self.groups, width, cands + 1)
        parents, ids = np.full([self.groups * width], -1, dtype=np.int64), np.full([self.groups * width], -1, dtype=np.int64)
        cum = np.full([self.groups * width], -np.inf)
        for g in range(self.groups):
            if self.done[g]:
                continue
            first, old, length = g * width, self.tokens[g], self.steps[g] + 1
            new, placed, used = [None] * width, 0, -1
            for p, (score, slot, token) in enumerate(top[g][:cands]):
                if self.eos is not None and token == self.eos:
                    if p < width:
                        self._keep(g, score / length ** self.length_penalty, old[slot - first] + [token])
                        used = p
                elif placed < width:
                    parents[first + placed], ids[first + placed], cum[first + placed] = slot, token, score
                    new[placed] = old[slot - first] + [token]
                    placed, used = placed + 1, p
            if self.eos is not None and width < len(top[g]) and self.eos in (top[g][width - 1][2], top[g][width][2]):
                used = max(used, width - 1)                                # whether eos sits below position W was decided there
            decisive = top[g][:used + 2]                                   # the candidates used, and the first one that was not
            self.gaps += [a[0] - b[0] for a, b in zip(decisive, decisive[1:])]
            self.scores_seen += [a[0] for a in decisive]
            self.tokens[g], self.steps[g] = new, length
            if placed == 0:
                self.done[g] = True
            elif len(self.hyps[g]) >= width:
                best = cum[first] / length ** self.length_penalty
                if not self.early_stopping:
                    self.gaps.append(abs(best - self.hyps[g][-1][0]))
                self.done[g] = self.early_stopping or best <= self.hyps[g][-1][0]
            if not self.done[g] and self.max_new_tokens is not None and length >= self.max_new_tokens:
                for j in range(placed):
                    self._keep(g, cum[first + j] / length ** self.length_penalty, new[j])
                self.done[g] = True
            if self.done[g]:
                parents[first:first + width], ids[first:first + width], cum[first:first + width] = -1, -1, -np.inf
                self.tokens[g] = [None] * width
        self.cum = cum
        return parents, ids, np.array(self.done)
