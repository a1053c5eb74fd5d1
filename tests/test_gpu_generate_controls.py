"""GPU: generation with logit processors end to end -- the plain loop ``proc(logits, history) -> sampler(logits) ->
history.append(result)`` against ``speculative.decode_step(..., processor=proc)`` on the fixture of tests/controls_cases.py
(the decoder, embedding and head of tests/spec_cases.py; seed 7, chosen on the host simulator, where tests/test_logits_host.py
asserts a least top-2 gap of 5e-3).

Greedy slots: slot 0 with repetition and frequency penalties, slot 1 with a bias list that bans a token it would otherwise emit,
slot 2 with an eos it would otherwise emit among its first three tokens and ``min_new_tokens`` 3.  The logits of a T + 1 chunk and
of single steps agree to the decode tests' 1e-5 (scaled), not bitwise, so each run first asserts from the plain loop's own
PROCESSED logits that every top-2 gap is at least 1e-3 of max |logit| -- 100 times that tolerance, the margin of
tests/test_gpu_spec.py -- and then that the speculative tokens EQUAL the plain ones.  The assertion fails loudly; nothing skips.

Needs ``LogitProcessor``, ``TokenHistory``, ``logprobs`` and ``decode_step(processor=)``: does not pass on the parent commit.
"""

import numpy as np
import pytest

import controls_cases as GC
import spec_cases as XC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.mark.parametrize('cache_dtype', ['f32', 'f16'])
def test_greedy_generation_with_processors_speculative_equals_plain(npm, cache_dtype):
    from np_modeling_amd import _C
    model = XC.make_model(npm, seed=GC.SEED)
    checked = []

    def keep(logits, result):
        """The log-probability of a greedy token is the first entry of the top list, bit for bit."""
        out = npm.sampling.logprobs(logits, ids=result.ids, top_n=3)
        assert np.array_equal(out.chosen.view(np.uint32), out.top_logprobs[:, 0].view(np.uint32))
        assert out.top_tokens[:, 0].tolist() == result.numpy().tolist() and (out.chosen <= 0).all()
        checked.append(out.lse)

    want, logits, history = GC.plain(npm, model, npm.sampling.Sampler(3), GC.processor(npm), cache_dtype=cache_dtype, keep=keep)
    gap = GC.least_gap(logits)
    print(f'controls {cache_dtype}: least top-2 gap of the processed plain run {gap:.3e} of max |logit|')
    assert gap >= GC.GAP, 'the fixture has a near-tie: chunked and single-step logits may pick different tokens'
    assert len(checked) == GC.EMIT and np.isfinite(np.array(checked)).all()
    bare, _, _ = GC.plain(npm, model, npm.sampling.Sampler(3), None, cache_dtype=cache_dtype)
    assert GC.BANNED in bare[1] and GC.EOS in bare[2][:GC.MIN_NEW], 'without the processor the rules would change nothing'
    assert all(z[1, GC.BANNED] == -np.inf for z in logits) and all(z[2, GC.EOS] == -np.inf for z in logits[:GC.MIN_NEW])
    assert all(z[2, GC.EOS] > -np.inf for z in logits[GC.MIN_NEW:])

    sampler = npm.sampling.Sampler(3)
    got, log, state, drafter = GC.speculative(npm, model, sampler, GC.processor(npm), cache_dtype=cache_dtype)
    assert 'logits_process_kernel B=3 rows=5 V=50 history=1 bias=2' == _C.last_logits_kernel()
    accepted, rejected = XC.accepts_and_rejects(log)
    print(f'controls {cache_dtype}: {len(log)} steps for {[len(g) for g in got]} tokens, slot-steps accepting {accepted}, rejecting {rejected}')
    assert [g[:GC.EMIT] for g in got] == want and np.array(want).shape == (3, GC.EMIT)
    assert accepted >= 1 and rejected >= 1 and len(log) < GC.EMIT - 1
    assert GC.BANNED not in got[1] and GC.EOS not in got[2][:GC.MIN_NEW]
    emitted = np.array([len(g) for g in got])
    assert sampler.draw.tolist() == emitted.tolist() == sampler.device_draw().tolist()
    assert drafter.device_lengths().tolist() == (np.array(XC.PROMPT_LENGTHS) + emitted).tolist() == drafter.lengths.tolist()
    lines = drafter.numpy()
    for b in range(3):
        assert lines[b, :drafter.lengths[b]].tolist() == model[4][b] + got[b]
        assert history.numpy()[b, :history.lengths[b]].tolist() == model[4][b] + want[b]
