"""TEST INFRASTRUCTURE ONLY -- the generation fixture shared by tests/test_spec_host.py (host simulator) and tests/test_gpu_spec.py
(MI355X), on the recipe of tests/test_gpu_generate.py: F 32, 2 heads, hidden 64, vocabulary 50, a paged cache of 16-row pages,
three prompts of different lengths -- repetitive ones here, so that prompt lookup has something to find -- and two loops over it:
``plain`` emits one token per step through ``sampler(logits)``, ``speculative`` several through ``speculative.decode_step``."""

import numpy as np

import decode_cases as DC

F, HEADS, HIDDEN, VOCAB, PAGE, CAPACITY, MAX_DRAFT, EMIT = 32, 2, 64, 50, 16, 48, 4, 12
PROMPT_LENGTHS = (9, 4, 6)
SEED = 4                       # chosen on the host simulator: tests/test_spec_host.py asserts what the GPU test needs of it
GAP = 1e-3                     # the least top-2 gap of a plain run's logits, relative to max |logit|: 100 x the decode tests' 1e-5


def make_model(npm, seed=SEED, window=None):
    """(decoder, embedding, head, memory [3, 7, F], prompts): the decoder as ``decode_cases.make_decoder`` scales it."""
    np.random.seed(seed)
    dec = npm.layers.TransformerDecoder(num_heads=HEADS, hidden_units=HIDDEN, norm_first=True, num_kv_heads=HEADS, causal=True,
                                        window=window)
    dec(np.zeros([3, 2, F], dtype=np.float32), np.zeros([3, 7, F], dtype=np.float32))
    for path, attrs in (('_self_attention', ('_wq', '_wk', '_wv', '_wo')), ('_cross_attention', ('_wq', '_wk', '_wv', '_wo')),
                        ('_dense1._linear', ('_w',)), ('_dense2', ('_w',))):
        for attr in attrs:
            arr = getattr(DC.sub(dec, path), attr)
            arr.set(np.asarray(arr) * np.float32(2.0 / np.sqrt(F)))
    emb = npm.layers.Embedding(VOCAB, F)
    emb(np.zeros([1], dtype=np.int64))
    head = npm.layers.Linear(units=VOCAB)
    head(np.zeros([1, F], dtype=np.float32))
    head._w.set(np.asarray(head._w) * np.float32(2.0 / np.sqrt(F)))
    rng = np.random.default_rng(seed + 1)
    kv = rng.standard_normal([3, 7, F]).astype(np.float32)
    prompts = []
    for n in PROMPT_LENGTHS:                                             # a period of 2 or 3 tokens, repeated
        period = rng.choice(VOCAB, size=int(rng.integers(2, 4)), replace=False)
        prompts.append([int(period[i % period.size]) for i in range(n)])
    return dec, emb, head, kv, prompts


def _prefill(npm, model, rows, sampler, cache_dtype, capacity):
    """The prompts through ``decode`` and the first token of every sequence; (state, first tokens, the logits they came from)."""
    from np_modeling_amd import device as D
    dec, emb, head, kv, prompts = model
    lengths = np.array([len(prompts[b]) for b in rows])
    batch, width = len(rows), int(lengths.max())
    state = dec.start_decoding(kv[list(rows)], capacity, page_size=PAGE, pages=batch * -(-capacity // PAGE), cache_dtype=cache_dtype)
    padded = np.full([batch, width], -1, dtype=np.int64)
    for i, b in enumerate(rows):
        padded[i, :lengths[i]] = prompts[b]
    hidden = dec.decode(emb.forward(padded), state, new_lengths=lengths)
    logits = head(D.take_rows(hidden.reshape(-1, F), np.arange(batch) * width + lengths - 1))
    return state, sampler(logits), logits.numpy()


def plain(npm, model, sampler, rows=(0, 1, 2), cache_dtype='f32', emit=EMIT, capacity=CAPACITY):
    """``emit`` tokens per sequence, one per step.  (tokens [B][emit], the logits of every step, pages in use, cache lengths)."""
    dec, emb, head, _, _ = model
    batch = len(rows)
    state, result, first_logits = _prefill(npm, model, rows, sampler, cache_dtype, capacity)
    tokens, logits = [result.numpy().tolist()], [first_logits]
    for _ in range(emit - 1):
        hidden = dec.decode(emb.forward(result.ids).reshape(batch, 1, F), state)
        z = head(hidden.reshape(batch, F))
        result = sampler(z)
        tokens.append(result.numpy().tolist())
        logits.append(z.numpy())
    return np.array(tokens).T.tolist(), logits, state.self_cache.pages_in_use, state.self_cache.lengths.copy()


def speculative(npm, model, sampler, rows=(0, 1, 2), cache_dtype='f32', emit=EMIT, ngram=(3, 1), probe=None, capacity=CAPACITY):
    """At least ``emit`` tokens per sequence through ``speculative.decode_step``; a sequence that has them sits the later steps out.
    (tokens [B][>= emit], what every ``Sampler.verify`` was given and found as (n_draft [B], accepted [B]), state, drafter).
    ``probe``: a counter read before and after every step; its growth per step becomes the third entry of that step's record."""
    dec, emb, head, _, prompts = model
    batch = len(rows)
    state, result, _ = _prefill(npm, model, rows, sampler, cache_dtype, capacity)
    first = result.numpy().tolist()
    drafter = npm.sampling.NgramDrafter(batch, max(PROMPT_LENGTHS) + emit + MAX_DRAFT, MAX_DRAFT, ngram=ngram)
    tokens = [[first[i]] for i in range(batch)]
    for i, b in enumerate(rows):
        drafter.admit(i, prompts[b] + [first[i]])
    verify, log = sampler.verify, []

    def recording(logits, draft, n_draft, **kwargs):
        found = verify(logits, draft, n_draft, **kwargs)
        log.append((np.asarray(n_draft).copy(), found.accepted))
        return found

    sampler.verify = recording
    try:
        while min(len(t) for t in tokens) < emit:
            active = np.array([len(t) < emit for t in tokens])
            before, history = state.self_cache.lengths.copy(), drafter.lengths.copy()
            count = probe() if probe else 0
            out = npm.speculative.decode_step(dec, state, emb, head, sampler, drafter, active=active)
            if probe:
                log[-1] += (probe() - count,)
            grown = drafter.lengths - history
            assert [len(o) for o in out] == grown.tolist() and (state.self_cache.lengths - before == grown).all()
            assert all((len(o) >= 1) == bool(a) for o, a in zip(out, active))
            for i in range(batch):
                tokens[i] += out[i]
            assert len(log) <= emit
    finally:
        del sampler.verify
    return tokens, log, state, drafter


def least_gap(logits) -> float:
    """The least top-2 gap over the rows of a plain run's logits, relative to the row's max |logit|."""
    gaps = []
    for z in logits:
        top = np.sort(z, axis=1)
        gaps.append(float(((top[:, -1] - top[:, -2]) / np.abs(z).max(axis=1)).min()))
    return min(gaps)


def accepts_and_rejects(log):
    """(slots-steps in which at least one drafted token was accepted, slot-steps in which one was rejected)."""
    accepted = sum(int(((n >= 0) & (a > 0)).sum()) for n, a, *_ in log)
    rejected = sum(int(((n >= 0) & (a < n)).sum()) for n, a, *_ in log)
    return accepted, rejected


# ---- hand-worked histories: (history, T, limit, (nmax, nmin), (n, j, m), chunk) ------------------------------------------------------
HAND = {
    # nothing occurs twice: n = 3, 2, 1 all without a candidate
    'no match': ([1, 2, 3, 4, 5], 4, 4, (3, 1), (None, None, 0), [5, -1, -1, -1, -1]),
    # [7 8 9] occurred at j = 0 only; 0 + 3 + 2 <= 8, the draft is h[3], h[4]
    'one match': ([7, 8, 9, 1, 2, 7, 8, 9], 2, 2, (3, 1), (3, 0, 2), [9, 1, 2]),
    # [1 2] at j = 0, 4, 8; T = 2: all three have a whole continuation (j <= 9), the most recent wins: h[10], h[11]
    'several, recent': ([1, 2, 5, 6, 1, 2, 7, 8, 1, 2, 9, 1, 2], 2, 2, (2, 1), (2, 8, 2), [2, 9, 1]),
    # the same with T = 4: j + 2 + 4 <= 13 leaves j = 0, 4; the largest of THOSE: h[6 .. 9]
    'several, whole': ([1, 2, 5, 6, 1, 2, 7, 8, 1, 2, 9, 1, 2], 4, 4, (2, 1), (2, 4, 4), [2, 7, 8, 1, 2]),
    # a b a b a b: [b a b] at j = 1 only, overlapping the tail; 1 + 3 + 4 > 6, so the smallest candidate, m = 6 - 4 = 2
    'periodic': ([1, 2, 1, 2, 1, 2], 4, 4, (3, 1), (3, 1, 2), [2, 1, 2, -1, -1]),
    # a b x 4, T = 7: [b a b] at j = 1, 3, none with 7 tokens behind it: the smallest, j = 1, m = 8 - 4 = 4
    'periodic, smallest': ([1, 2] * 4, 7, 7, (3, 1), (3, 1, 4), [2, 1, 2, 1, 2, -1, -1, -1]),
    # ... and T = 2: j + 3 + 2 <= 8 holds for both, the largest, j = 3: h[6], h[7]
    'periodic, largest': ([1, 2] * 4, 2, 2, (3, 1), (3, 3, 2), [2, 1, 2]),
    # L = 3 < nmax + 1: n = 3 is skipped; [5 4] never occurred; [4] at j = 0, and only 2 tokens follow it
    'short continuation': ([4, 5, 4], 3, 3, (3, 1), (1, 0, 2), [4, 5, 4, -1]),
    # nmax = 3 finds nothing, nmin = 2 does: [2 3] at j = 1, followed by 9
    'nmin hits': ([1, 2, 3, 9, 2, 3], 1, 1, (3, 2), (2, 1, 1), [3, 9]),
    # the limit cuts the draft: 1 token, none, and an inactive slot
    'limit 1': ([7, 8, 9, 1, 2, 7, 8, 9], 2, 1, (3, 1), (3, 0, 1), [9, 1, -1]),
    'limit 0': ([7, 8, 9, 1, 2, 7, 8, 9], 2, 0, (3, 1), (None, None, 0), [9, -1, -1]),
    'limit -1': ([7, 8, 9, 1, 2, 7, 8, 9], 2, -1, (3, 1), (None, None, 0), [-1, -1, -1]),
    # L = 0, 1, n, n + 1 with n = 3 alone: inactive; no n fits (twice); one candidate, j = 0, and one token behind it
    'L 0': ([], 2, 2, (3, 3), (None, None, 0), [-1, -1, -1]),
    'L 1': ([5], 2, 2, (3, 3), (None, None, 0), [5, -1, -1]),
    'L n': ([5, 5, 5], 2, 2, (3, 3), (None, None, 0), [5, -1, -1]),
    'L n + 1': ([5, 5, 5, 5], 2, 2, (3, 3), (3, 0, 1), [5, 5, -1]),
}
