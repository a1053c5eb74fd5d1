"""GPU: the generation loop closed on the device -- sampler -> ``Embedding.forward(result.ids)`` -> ``TransformerDecoder.decode`` on
a paged cache -> ``device.take_rows`` of every sequence's last row -> the vocabulary projection -- against the same loop with the
logits copied to the host, ``np.argmax`` there and the embedding rows uploaded.

Bounds: none.  Both paths run the same kernels on the same device values; greedy over the same device logits leaves no room
for a margin, so tokens are equal and embedded rows are compared as uint32.  The sampled run compares tokens only.

Every test here needs ``sampling.Sampler``, ``layers.Embedding`` and ``device.take_rows``: none passes on the parent commit.
"""

import numpy as np
import pytest

import decode_cases as DC

pytestmark = pytest.mark.gpu

F, HEADS, HIDDEN, VOCAB, STEPS = 32, 2, 64, 50, 6
PROMPTS = (5, 1, 3)


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.fixture(scope='module')
def model(npm):
    dec, _ = DC.make_decoder(npm, F, HEADS, HEADS, HIDDEN, norm_first=True, causal=True, seed=40, batch=3, seq_kv=7)
    np.random.seed(41)
    emb = npm.layers.Embedding(VOCAB, F)
    emb(np.zeros([1], dtype=np.int64))
    head = npm.layers.Linear(units=VOCAB)
    head(np.zeros([1, F], dtype=np.float32))
    head._w.set(np.asarray(head._w) * np.float32(2.0 / np.sqrt(F)))                 # logits about a unit apart
    rng = np.random.default_rng(42)
    kv = rng.standard_normal([3, 7, F]).astype(np.float32)
    prompt = np.full([3, max(PROMPTS)], -1, dtype=np.int64)                          # -1: a row of zeros, finite padding
    for b, n in enumerate(PROMPTS):
        prompt[b, :n] = rng.integers(0, VOCAB, size=n)
    return dec, emb, head, kv, prompt


def _generate(npm, model, rows, on_device, sampler=None):
    """STEPS tokens for the sequences ``rows``; (tokens [STEPS, B], the embedded rows fed back at every step)."""
    from np_modeling_amd import device as D
    dec, emb, head, kv, prompt = model
    rows = list(rows)
    lengths = np.array([PROMPTS[b] for b in rows])
    batch, width = len(rows), int(lengths.max())
    state = dec.start_decoding(kv[rows], 16, page_size=16, pages=batch)
    table = emb.w.numpy()
    x = emb.forward(prompt[rows][:, :width])
    new_lengths, last = lengths, np.arange(batch) * width + lengths - 1
    tokens, fed = [], []
    for step in range(STEPS):
        hidden = dec.decode(x, state, new_lengths=new_lengths)
        logits = head(D.take_rows(hidden.reshape(-1, F), last))
        if on_device:
            result = sampler(logits)
            x = emb.forward(result.ids).reshape(batch, 1, F)
            ids = result.numpy()
        else:
            ids = np.argmax(logits.numpy(), axis=1)
            x = D.from_host(table[ids]).reshape(batch, 1, F)
        tokens.append(np.asarray(ids).tolist())
        fed.append(x.numpy().view(np.uint32))
        new_lengths, last = None, np.arange(batch)
    assert state.self_cache.lengths.tolist() == (lengths + STEPS - 1).tolist()
    return np.array(tokens), fed


def test_greedy_tokens_on_the_device_are_the_host_argmax_loop(npm, model):
    device_tokens, device_fed = _generate(npm, model, range(3), True, npm.sampling.Sampler(3))
    host_tokens, host_fed = _generate(npm, model, range(3), False)
    assert device_tokens.shape == (STEPS, 3) and np.array_equal(device_tokens, host_tokens)
    assert all(np.array_equal(a, b) for a, b in zip(device_fed, host_fed))
    assert ((device_tokens >= 0) & (device_tokens < VOCAB)).all() and len(np.unique(device_tokens)) > 3


def test_a_sampled_sequence_alone_yields_its_tokens_in_the_batch(npm, model):
    sampler = npm.sampling.Sampler(3)
    for b in range(3):
        sampler.set(b, temperature=0.8, top_k=10, seed=100 + b)
    in_batch, _ = _generate(npm, model, range(3), True, sampler)
    assert sampler.draw.tolist() == [STEPS] * 3 and sampler.device_draw().tolist() == [STEPS] * 3
    alone = npm.sampling.Sampler(1)
    alone.set(0, temperature=0.8, top_k=10, seed=101)
    tokens, _ = _generate(npm, model, [1], True, alone)
    assert tokens[:, 0].tolist() == in_batch[:, 1].tolist()
    greedy, _ = _generate(npm, model, range(3), True, npm.sampling.Sampler(3))
    assert not np.array_equal(greedy, in_batch)                                    # the draws did sample
