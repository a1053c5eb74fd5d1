"""GPU: the logit processors -- npm_logits_process and npm_history_append through the C ABI, and ``LogitProcessor`` /
``TokenHistory`` on the device.

Bounds: none anywhere.  The kernel's arithmetic is fp32 operation by fp32 operation what tests/logits_reference.py does in NumPy
float32 scalars (no contraction, IEEE division), so the logits are compared as uint32 -- over the WHOLE padded buffer: guard
words in front and behind, the pitch padding, the rows of inactive slots (filled with NaN) and the rows behind a draft, so that an
element the contract leaves alone is checked as unwritten.  One exception, stated in the reference: where a step applied and the
reference holds a NaN, any NaN will do (IEEE leaves the sign and payload of a NaN an operation produces open; every such element
is one of the special values the case put there).  After every call the workspace is all zero between its guard words and every
input array kept its bits (tests/logits_cases.py ``run``).

Every test here needs npm_logits_process, npm_history_append, ``LogitProcessor`` or ``TokenHistory``: none passes on the parent
commit.
"""

import ctypes as C

import numpy as np
import pytest

import logits_cases as LC
import logits_reference as LR

pytestmark = pytest.mark.gpu

GUARD, S32 = 8, 0x5A5A5A5A


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.mark.parametrize('name', sorted(LC.CASES))
def test_npm_logits_process_equals_the_reference_as_bits(npm, name):
    from np_modeling_amd import _C
    case = LC.CASES[name]()
    got = LC.check(case)
    assert _C.last_logits_kernel() == (f'logits_process_kernel B={case["batch"]} rows={case["rows"]} V={case["vocab"]} history=1 '
                                       f'bias={case["bias_cap"]}')
    assert np.array_equal(got, LC.run(case)), 'the same call on fresh inputs gave other bits'
    if name.startswith('shapes'):                       # a 16-byte aligned base and a pitch equal to the vocabulary
        LC.check(dict(case, front=4, pitch=case['vocab']))


@pytest.mark.parametrize('name', ['shapes-V63', 'drafts-rows8', 'bias-lists', 'minimum-length'])
def test_a_slot_is_the_batch_one_call_and_a_row_the_one_row_call_with_the_draft_prefix_appended(npm, name):
    case = LC.CASES[name]()
    whole = LC.body(case, LC.run(case))
    rows = case['rows']
    for b in LC.live_slots(case):
        alone = LC.slot_of(case, b)
        assert np.array_equal(LC.body(alone, LC.run(alone)), whole[b * rows:(b + 1) * rows]), b
        for r in range(min(int(case['n_draft'][b]), rows - 1) + 1):
            single = LC.row_of(case, b, r)
            assert np.array_equal(LC.body(single, LC.run(single))[0], whole[b * rows + r]), (b, r)


def test_null_pointers_mean_the_defaults(npm):
    """No history, no parameter vectors, no n_draft: only the bias list acts; without it too the call changes nothing."""
    case = LC.with_bias(LC.make(2, 1, 257, 5, [9, 9]), [[(3, 0.5), (256, -np.inf)], [(0, -0.25)]])
    bare = dict(case, history=None, history_len=None, prompt_len=None, n_draft=None, repetition=None, presence=None, frequency=None,
                eos=None, min_new=None)
    want, written = LC.expected(bare)
    assert written.sum() == 3 and LR.same(LC.run(bare).view(np.float32), want.view(np.float32), written)
    nothing = dict(bare, bias_index=None, bias_value=None, bias_count=None, bias_cap=0)
    assert np.array_equal(LC.run(nothing), LC.host_image(nothing))
    only_eos = dict(case, eos=np.array([7, 300], dtype=np.int32), min_new=None)            # eos without min_new: no rule
    want, written = LC.expected(only_eos)
    assert LR.same(LC.run(only_eos).view(np.float32), want.view(np.float32), written)


def test_npm_logits_process_refuses_bad_arguments_before_any_launch(npm):
    from np_modeling_amd import _C, device as D
    buf = D.zeros([256])
    ok = dict(logits=buf.ptr, pitch=4, batch=2, rows=2, vocab=4, history_cap=4, history=buf.ptr, history_pitch=4, history_len=buf.ptr,
              prompt_len=buf.ptr, draft=buf.ptr, draft_pitch=1, n_draft=buf.ptr, active=None, repetition=buf.ptr, presence=buf.ptr,
              frequency=buf.ptr, eos=buf.ptr, min_new=buf.ptr, bias_index=buf.ptr, bias_value=buf.ptr, bias_count=buf.ptr, bias_cap=2,
              workspace=buf.ptr)
    assert _C.lib().npm_logits_process(C.byref(_C.npm_logits(**ok))) == 0                 # all zero: neutral, nothing changes
    before = _C.last_logits_kernel()
    marker = D.ids_from_host(np.zeros([1], dtype=np.int32))
    _C.check(_C.lib().npm_history_append(marker.ptr, 1, 1, marker.ptr, marker.ptr, None, 1), 'npm_history_append')
    marked = _C.last_logits_kernel()
    assert marked != before
    for change in (dict(logits=None), dict(workspace=None), dict(batch=0), dict(rows=0), dict(rows=65), dict(vocab=0),
                   dict(vocab=(1 << 20) + 1), dict(pitch=3), dict(batch=2 ** 30, rows=2), dict(n_draft=None), dict(draft=None),
                   dict(draft_pitch=0), dict(history_len=None), dict(history_cap=0), dict(history_pitch=3), dict(bias_cap=-1),
                   dict(bias_cap=257), dict(bias_index=None), dict(bias_value=None), dict(bias_count=None)):
        assert _C.lib().npm_logits_process(C.byref(_C.npm_logits(**{**ok, **change}))) == 10002, change
    assert _C.lib().npm_logits_process(None) == 10002 and _C.last_logits_kernel() == marked
    for change in (dict(batch=0), dict(history_cap=0), dict(history_pitch=0), dict(history=None), dict(history_len=None), dict(ids=None)):
        args = {**dict(history=buf.ptr, history_pitch=1, history_cap=1, history_len=buf.ptr, ids=buf.ptr, active=None, batch=1), **change}
        assert _C.lib().npm_history_append(*args.values()) == 10002, change
    assert np.array_equal(buf.numpy(), np.zeros([256], dtype=np.float32))


def _guarded(D, values, dtype=np.uint32):
    host = np.full([np.asarray(values).size + 2 * GUARD], S32, dtype=np.uint32)
    host[GUARD:-GUARD] = np.asarray(values).reshape(-1).view(np.uint32)
    buf = D.bytes_from_host(host)
    return buf, buf.ptr + 4 * GUARD


def _inside(buf, what):
    host = buf.numpy().view(np.uint32)
    assert (host[:GUARD] == S32).all() and (host[-GUARD:] == S32).all(), f'a guard word around {what} was written'
    return host[GUARD:-GUARD].view(np.int32).copy()


@pytest.mark.parametrize('with_active', [False, True])
def test_npm_history_append(npm, with_active):
    """Lengths 0, cap - 1, cap, below 0 and above cap; id -1; active 0; a pitch above the capacity; guard words around both."""
    from np_modeling_amd import _C, device as D
    cap, pitch = 6, 8
    lengths = np.array([0, cap - 1, cap, -3, cap + 4, 2, 3], dtype=np.int32)
    ids = np.array([11, 12, 13, 14, 15, -1, 2 ** 31 - 1], dtype=np.int32)
    active = np.array([1, 1, 1, 7, 1, 1, 0], dtype=np.int32) if with_active else None
    batch = lengths.size
    lines = np.full([batch, pitch], -9, dtype=np.int32)
    hist, hist_ptr = _guarded(D, lines)
    lens, lens_ptr = _guarded(D, lengths)
    ids_dev = D.bytes_from_host(ids)
    active_dev = None if active is None else D.bytes_from_host(active)
    _C.check(_C.lib().npm_history_append(hist_ptr, pitch, cap, lens_ptr, ids_dev.ptr, None if active is None else active_dev.ptr, batch),
             'npm_history_append')
    assert _C.last_logits_kernel() == f'history_append_kernel B={batch} cap={cap}'
    want_lines, want_lengths = lines.copy(), lengths.copy()
    LR.history_append(want_lines, want_lengths, cap, ids, active)
    assert want_lengths.tolist() == [1, cap, cap, 1, cap + 4, 2, 3 if with_active else 4]
    assert np.array_equal(_inside(hist, 'history').reshape(batch, pitch), want_lines)
    assert np.array_equal(_inside(lens, 'history_len'), want_lengths)
    assert np.array_equal(ids_dev.numpy().view(np.int32), ids)


def test_logit_processor_and_token_history_on_the_device(npm):
    """The Python layer end to end on the device: a chunk call equals the reference, the workspace the object owns is zero again,
    a neutral processor launches nothing, and ``append`` keeps the host mirror equal to the device."""
    import math
    from np_modeling_amd import _C, device as D
    S = npm.sampling
    vocab, rows = 300, 3
    proc = S.LogitProcessor(2, vocab, max_bias=4)
    history = S.TokenHistory(2, 12)
    history.admit(0, [5, 9, 5, 200])
    history.admit(1, [299])
    z = (3 * np.random.default_rng(8).standard_normal([2 * rows, vocab])).astype(np.float32)
    marked = _C.last_logits_kernel()
    assert proc(D.from_host(z), history, draft=np.array([[9, 9], [1, -1]]), n_draft=[2, 1]).numpy().tobytes() == z.tobytes()
    assert _C.last_logits_kernel() == marked                            # neutral: nothing was launched
    proc.set(0, repetition_penalty=1.3, presence_penalty=0.7, frequency_penalty=0.1, logit_bias={7: -math.inf}, eos=200, min_new_tokens=4,
             prompt_length=2)
    proc.set(1, frequency_penalty=0.1, logit_bias={299: 0.5, 0: -1.5})
    draft, n_draft = np.array([[9, 9], [1, -1]], dtype=np.int32), np.array([2, 1], dtype=np.int32)
    want = z.copy()
    LR.process(want, 2, rows, vocab, history=history.numpy(), history_len=[4, 1], history_cap=12, prompt_len=[2, 0], draft=draft,
               n_draft=n_draft, repetition=[1.3, 1.0], presence=[0.7, 0.0], frequency=[0.1, 0.1], eos=[200, -1], min_new=[4, 0],
               bias_index=proc.bias_index, bias_value=proc.bias_value, bias_count=proc.bias_count, bias_cap=4)
    logits = D.from_host(z)
    assert proc(logits, history, draft=draft, n_draft=n_draft) is logits
    assert np.array_equal(logits.numpy().view(np.uint32), want.view(np.uint32)) and (want != z).sum() >= 8
    assert _C.last_logits_kernel() == f'logits_process_kernel B=2 rows={rows} V={vocab} history=1 bias=4'
    assert not proc._workspace.numpy().any()
    sampler = S.Sampler(2)
    result = sampler(D.from_host(z[::rows].copy()))
    history.append(result)
    tokens = result.numpy()
    assert history.lengths.tolist() == [5, 2] == history.device_lengths().tolist()
    assert history.numpy()[0, :5].tolist() == [5, 9, 5, 200, tokens[0]] and history.numpy()[1, :2].tolist() == [299, tokens[1]]
