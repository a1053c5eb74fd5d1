"""TEST INFRASTRUCTURE ONLY -- the decoder-only language model fixture shared by tests/test_lm_host.py (host simulator) and
tests/test_gpu_lm.py (MI355X): F 32, 2 heads over 1 key / value head, hidden 48, vocabulary 50, 3 layers, B 3, S 6 with ragged
lengths (6, 3, 5); rms + swiglu + rope by default.

* ``make_lm``: a seeded ``models.CausalLM`` with its matrices scaled to O(1) activations;
* ``reference_step``: logits, mean cross-entropy and every parameter gradient of one training step in float64 -- the blocks out
  of tests/llama_reference.py's norm and feed-forward and tests/rope_reference.py's rotating attention, NumPy for the embedding,
  the final norm, the head and the loss;
* ``greedy`` / ``speculative`` / ``beam``: the one-token loop through ``lm.decode``, and ``speculative.decode_step`` /
  ``beam.decode_step`` over ``lm.stack``, in the manner of tests/spec_cases.py and tests/beam_cases.py."""

import numpy as np

import beam_reference as BR
import llama_reference as LR
import rope_reference as RP

F, HEADS, HKV, HIDDEN, VOCAB, LAYERS, B, S = 32, 2, 1, 48, 50, 3, 3, 6
LENGTHS = (6, 3, 5)
ROPE_BASE = 10000.0
PROMPTS = (5, 3, 4)
SEED = 35                      # chosen on the host simulator: tests/test_lm_host.py asserts the top-2 gap the GPU test needs of it
LAYER_TOL = 1e-5               # tests/test_gpu_decode.py: decode against forward, relative to max |logit|
GAP = 100 * LAYER_TOL          # the GAP rule of tests/test_gpu_spec.py


def make_lm(npm, seed=SEED, layers=LAYERS, **keywords):
    """A ``CausalLM`` at the shared shape, parameters drawn from ``seed`` by one forward, every matrix of the blocks and the head
    times 2 / sqrt(F) (written in place: the arenas stay what they are)."""
    np.random.seed(seed)
    lm = npm.models.CausalLM(VOCAB, F, layers, HEADS, HIDDEN, num_kv_heads=HKV, **keywords)
    lm(np.zeros([B, 2], dtype=np.int64))
    for block in lm.layers:
        for owner, attribute in LR.parameters(block).values():
            value = owner._param(attribute)
            if value.ndim > 1:
                value.set(np.asarray(value) * np.float32(2.0 / np.sqrt(F)))
    lm.head._w.set(np.asarray(lm.head._w) * np.float32(2.0 / np.sqrt(F)))
    return lm


def tokens(seed=SEED + 1):
    """(tokens [B, S + 1] padded with -1, inputs [B, S], targets [B, S]): sequence b has LENGTHS[b] + 1 tokens, none twice."""
    rng = np.random.default_rng(seed)
    full = np.full([B, S + 1], -1, dtype=np.int64)
    for b, n in enumerate(LENGTHS):
        full[b, :n + 1] = rng.permutation(VOCAB)[:n + 1]
    inputs, targets = full[:, :-1].copy(), full[:, 1:].copy()
    for b, n in enumerate(LENGTHS):
        inputs[b, n:] = -1
        targets[b, n:] = -1
    return full, inputs, targets


def prompts(seed=SEED + 2):
    """[B, max(PROMPTS)] padded with -1: periods of 2 or 3 tokens, so that prompt lookup has something to find."""
    rng = np.random.default_rng(seed)
    out = np.full([B, max(PROMPTS)], -1, dtype=np.int64)
    for b, n in enumerate(PROMPTS):
        period = rng.choice(VOCAB, size=int(rng.integers(2, 4)), replace=False)
        out[b, :n] = [int(period[i % period.size]) for i in range(n)]
    return out


class Recorder:
    """An optimizer that keeps every gradient by (owner, attribute) and changes nothing."""

    def __init__(self):
        self.grads, self.order = {}, []

    def update(self, obj, attribute, gradient):
        self.grads[(id(obj), attribute)] = np.array(gradient, dtype=np.float64, copy=True)
        self.order.append(type(obj).__name__ + '.' + attribute)


# ---- float64 -------------------------------------------------------------------------------------------------------------------
def _f64(a):
    return np.asarray(a).astype(np.float64)


def reference_step(lm, inputs, targets, *, norm='rms', ffn='swiglu', norm_first=True, window=None):
    """(logits [B, S, V], loss, {(id(owner), attribute): gradient}) of the mean cross-entropy over the targets >= 0."""
    inputs, targets = np.asarray(inputs), np.asarray(targets)
    b, s = inputs.shape
    table = _f64(lm.embedding._w)
    x = np.where((inputs >= 0)[..., None], table[np.maximum(inputs, 0)], 0.0)
    mask = np.tril(np.ones([s, s], dtype=bool))
    if window is not None:
        mask &= ~np.tril(np.ones([s, s], dtype=bool), -window)
    backs = []
    for block in lm.layers:
        names = LR.parameters(block)
        p = LR.values(block)
        ap = {n: p['sa.' + n] for n in LR.ATT}
        if norm_first:
            z, norm1 = LR._norm(p, 'n1', x, norm, None)
            y, cache = RP.att_fwd(ap, ROPE_BASE, z, mask=mask)
            x1 = x + y
            z2, norm2 = LR._norm(p, 'n2', x1, norm, None)
            y2, ff = LR._feed_forward(p, z2, ffn)
            x = x1 + y2
        else:
            y, cache = RP.att_fwd(ap, ROPE_BASE, x, mask=mask)
            x1, norm1 = LR._norm(p, 'n1', x + y, norm, None)
            y2, ff = LR._feed_forward(p, x1, ffn)
            x, norm2 = LR._norm(p, 'n2', x1 + y2, norm, None)

        def back(dy, names=names, ap=ap, cache=cache, norm1=norm1, norm2=norm2, ff=ff):
            if norm_first:
                dz2, g_ff = ff(dy)
                dn2, g_n2 = norm2(dz2)
                d1 = dy + dn2
                (dq, dk, dv), g_att = RP.att_bwd(ap, cache, d1)
                dn1, g_n1 = norm1(dq + dk + dv)
                dx = d1 + dn1
            else:
                dn2, g_n2 = norm2(dy)
                dff, g_ff = ff(dn2)
                d1 = dn2 + dff
                dn1, g_n1 = norm1(d1)
                (dq, dk, dv), g_att = RP.att_bwd(ap, cache, dn1)
                dx = dn1 + dq + dk + dv
            grads = {**g_ff, **g_n1, **g_n2, **{'sa.' + n: g for n, g in g_att.items()}}
            return dx, {(id(names[k][0]), names[k][1]): g for k, g in grads.items()}
        backs.append(back)
    final = None
    if lm.final_norm is not None:
        fp = {'fn.gamma': _f64(lm.final_norm._gamma)}
        if hasattr(lm.final_norm, '_beta'):
            fp['fn.beta'] = _f64(lm.final_norm._beta)
        x, final = LR._norm(fp, 'fn', x, norm, None)
    hidden = x.reshape(b * s, F)
    w, bias = _f64(lm.head._w), _f64(lm.head._b)
    logits = hidden @ w + bias
    flat = targets.reshape(-1)
    live = flat >= 0
    top = logits.max(axis=1, keepdims=True)
    lse = top[:, 0] + np.log(np.exp(logits - top).sum(axis=1))
    loss = float((lse[live] - logits[live, flat[live]]).mean())
    dlogits = np.exp(logits - lse[:, None])
    dlogits[live, flat[live]] -= 1.0
    dlogits = np.where(live[:, None], dlogits, 0.0) / live.sum()
    grads = {(id(lm.head), '_w'): hidden.T @ dlogits, (id(lm.head), '_b'): dlogits.sum(axis=0)}
    dx = (dlogits @ w.T).reshape(b, s, F)
    if final is not None:
        dx, g = final(dx)
        grads[(id(lm.final_norm), '_gamma')] = g['fn.gamma']
        if 'fn.beta' in g:
            grads[(id(lm.final_norm), '_beta')] = g['fn.beta']
    for back in backs[::-1]:
        dx, g = back(dx)
        grads.update(g)
    dtable = np.zeros_like(table)
    np.add.at(dtable, inputs[inputs >= 0], dx[inputs >= 0])
    grads[(id(lm.embedding), '_w')] = dtable
    return logits.reshape(b, s, VOCAB), loss, grads


# ---- generation ----------------------------------------------------------------------------------------------------------------
def top2_gap(logits, live=None) -> float:
    """The least top-2 gap of the rows (``live``: a mask over them), relative to the largest |logit| of those rows."""
    z = np.asarray(logits, dtype=np.float64).reshape(-1, np.shape(logits)[-1])
    if live is not None:
        z = z[np.asarray(live).reshape(-1)]
    top = np.sort(z, axis=1)
    return float((top[:, -1] - top[:, -2]).min() / np.abs(z).max())


def greedy(npm, lm, steps, **start):
    """The one-token loop: (tokens [B, steps], the logits of every step, state)."""
    from np_modeling_amd import device as D
    prompt, lengths = prompts(), np.array(PROMPTS)
    state = lm.start_decoding(B, 24, **start)
    sampler = npm.sampling.Sampler(B)
    logits = lm.decode(prompt, state, new_lengths=lengths)
    out, seen = [], []
    for _ in range(steps):
        seen.append(logits.numpy())
        result = sampler(logits)
        out.append(result.numpy().tolist())
        logits = lm.decode(D.IdBuffer([B, 1], result.ids._buf, result.ids.ptr), state)
    return np.array(out).T, seen, state


def speculative(npm, lm, emit, max_draft=3, **start):
    """At least ``emit`` tokens per sequence through ``speculative.decode_step`` over ``lm.stack``: (tokens [B][>= emit], steps)."""
    prompt, lengths = prompts(), np.array(PROMPTS)
    state = lm.start_decoding(B, 24, **start)
    sampler = npm.sampling.Sampler(B)
    first = sampler(lm.decode(prompt, state, new_lengths=lengths)).numpy().tolist()
    drafter = npm.sampling.NgramDrafter(B, max(PROMPTS) + emit + max_draft, max_draft, ngram=(3, 1))
    out = [[first[b]] for b in range(B)]
    for b in range(B):
        drafter.admit(b, prompt[b, :PROMPTS[b]].tolist() + [first[b]])
    steps = 0
    while min(len(t) for t in out) < emit:
        active = np.array([len(t) < emit for t in out])
        emitted = npm.speculative.decode_step(lm.stack, state, lm.embedding, lm.head, sampler, drafter, active=active)
        for b in range(B):
            out[b] += emitted[b]
        steps += 1
        assert steps <= emit
    return out, steps


def beam(npm, lm, groups, width, max_new_tokens, eos=None, **start):
    """``beam.decode_step`` over ``lm.stack`` until every group is done, ``beam_reference.PyBeamSearch`` beside it on the logits of
    each step: (search, reference, the logits of every step)."""
    batch = groups * width
    state = lm.start_decoding(batch, 16, page_size=16, pages=2 * batch, **start)
    search = npm.beam.BeamSearch(groups, width, eos=eos, max_new_tokens=max_new_tokens)
    reference = BR.PyBeamSearch(groups, width, eos=eos, max_new_tokens=max_new_tokens)
    chunk, n = np.full([batch, max(PROMPTS)], -1, dtype=np.int64), np.zeros([batch], dtype=np.int64)
    chunk[::width], n[::width] = prompts()[:groups], PROMPTS[:groups]
    seen = []

    def spy(x):
        logits = lm.head(x)
        seen.append(logits.numpy())
        return logits

    first, done = (chunk, n), np.zeros([groups], dtype=bool)
    while not done.all():
        assert len(seen) <= max_new_tokens
        done = npm.beam.decode_step(lm.stack, state, lm.embedding, spy, search, prompt=first)
        first = None
        parents, ids, ref_done = reference.search(seen[-1])
        assert search.step.parents.tolist() == parents.tolist() and search.step.host_ids.tolist() == ids.tolist(), len(seen)
        assert done.tolist() == ref_done.tolist()
    return search, reference, seen
