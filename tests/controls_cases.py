"""TEST INFRASTRUCTURE ONLY -- the generation fixture with logit processors shared by tests/test_logits_host.py (host simulator) and
tests/test_gpu_generate_controls.py (MI355X): the model of tests/spec_cases.py (``make_model`` with the seed below), a
``LogitProcessor`` that gives slot 0 repetition and frequency penalties, slot 1 a bias list with one ban and slot 2 an eos that
may not appear among its first three tokens, and two loops over it:

``plain``        proc(logits, history) -> sampler(logits) -> history.append(result), one token a step;
``speculative``  ``speculative.decode_step(..., processor=proc)``, several tokens a step.

SEED, BANNED and EOS were chosen on the host simulator: without the processor the plain greedy loop emits BANNED in slot 1 and
EOS among the first three tokens of slot 2, so both rules change the run; tests/test_logits_host.py asserts what the GPU test
needs of the fixture.
"""

import math

import numpy as np

import spec_cases as XC

SEED = 7                               # least top-2 gap of the processed plain run on the simulator: 9.0e-3 (f32 and f16 caches)
EMIT = XC.EMIT
BANNED, EOS, MIN_NEW = 13, 45, 3       # slot 1's most frequent token and slot 2's second token in the run without a processor
GAP = 1e-3                             # the least top-2 gap of the plain run's processed logits over max |logit| (GPU test)
GAP_HOST = 5e-3                        # what the host test asserts of the seed, as tests/test_spec_host.py did for its own


def processor(npm):
    proc = npm.sampling.LogitProcessor(3, XC.VOCAB, max_bias=2)
    proc.set(0, repetition_penalty=1.15, frequency_penalty=0.05, prompt_length=XC.PROMPT_LENGTHS[0])
    proc.set(1, logit_bias={BANNED: -math.inf, (BANNED + 1) % XC.VOCAB: 0.125})
    proc.set(2, repetition_penalty=1.05, eos=EOS, min_new_tokens=MIN_NEW, prompt_length=XC.PROMPT_LENGTHS[2])
    return proc


def _prefill(npm, model, cache_dtype, capacity):
    """The prompts through ``decode``; (state, the logits of every sequence's last prompt row)."""
    from np_modeling_amd import device as D
    dec, emb, head, kv, prompts = model
    lengths = np.array([len(p) for p in prompts])
    batch, width = len(prompts), int(lengths.max())
    state = dec.start_decoding(kv, capacity, page_size=XC.PAGE, pages=batch * -(-capacity // XC.PAGE), cache_dtype=cache_dtype)
    padded = np.full([batch, width], -1, dtype=np.int64)
    for b in range(batch):
        padded[b, :lengths[b]] = prompts[b]
    hidden = dec.decode(emb.forward(padded), state, new_lengths=lengths)
    return state, head(D.take_rows(hidden.reshape(-1, XC.F), np.arange(batch) * width + lengths - 1))


def plain(npm, model, sampler, proc, cache_dtype='f32', emit=EMIT, capacity=XC.CAPACITY, keep=None):
    """``emit`` tokens per sequence, one a step.  (tokens [B][emit], the PROCESSED logits of every step, the history).
    ``keep(logits, result)`` is called with every step's processed device logits and its result."""
    dec, emb, head, _, prompts = model
    batch = len(prompts)
    history = npm.sampling.TokenHistory(batch, max(XC.PROMPT_LENGTHS) + emit)
    for b in range(batch):
        history.admit(b, prompts[b])
    state, z = _prefill(npm, model, cache_dtype, capacity)
    tokens, logits = [], []
    for step in range(emit):
        if step:
            z = head(dec.decode(emb.forward(result.ids).reshape(batch, 1, XC.F), state).reshape(batch, XC.F))
        if proc is not None:
            z = proc(z, history)
        result = sampler(z)
        if keep is not None:
            keep(z, result)
        history.append(result)
        tokens.append(result.numpy().tolist())
        logits.append(z.numpy())
    return np.array(tokens).T.tolist(), logits, history


def speculative(npm, model, sampler, proc, cache_dtype='f32', emit=EMIT, capacity=XC.CAPACITY, probe=None):
    """At least ``emit`` tokens per sequence through ``speculative.decode_step(..., processor=proc)``; the first token comes from
    the prompt's last row as in ``plain``.  (tokens [B][>= emit], per step (n_draft, accepted[, probe growth]), state, drafter)."""
    dec, emb, head, _, prompts = model
    batch = len(prompts)
    drafter = npm.sampling.NgramDrafter(batch, max(XC.PROMPT_LENGTHS) + emit + XC.MAX_DRAFT, XC.MAX_DRAFT)
    for b in range(batch):
        drafter.admit(b, prompts[b])
    state, z = _prefill(npm, model, cache_dtype, capacity)
    if proc is not None:
        z = proc(z, drafter)
    result = sampler(z)
    drafter.append(result)
    tokens = [[t] for t in result.numpy().tolist()]
    verify, log = sampler.verify, []

    def recording(logits, draft, n_draft, **kwargs):
        found = verify(logits, draft, n_draft, **kwargs)
        log.append((np.asarray(n_draft).copy(), found.accepted))
        return found

    sampler.verify = recording
    try:
        while min(len(t) for t in tokens) < emit:
            active = np.array([len(t) < emit for t in tokens])
            count = probe() if probe else 0
            out = npm.speculative.decode_step(dec, state, emb, head, sampler, drafter, active=active, processor=proc)
            if probe:
                log[-1] += (probe() - count,)
            for b in range(batch):
                tokens[b] += out[b]
            assert len(log) <= emit
    finally:
        del sampler.verify
    return tokens, log, state, drafter


def least_gap(logits) -> float:
    """The least top-2 gap over the rows of a run's processed logits, relative to the row's largest finite |logit| (a banned
    token's -inf is no near-tie)."""
    gaps = []
    for z in logits:
        top = np.sort(z, axis=1)
        scale = np.where(np.isfinite(z), np.abs(z), 0).max(axis=1)
        gaps.append(float(((top[:, -1] - top[:, -2]) / scale).min()))
    return min(gaps)
