"""CPU: the logit processors on the host simulator (tests/hostsim/ (profile 'logits')) and their reference (tests/logits_reference.py).

* the reference on hand-worked rows; the case lists of tests/logits_cases.py through the C-ABI runner on the simulator;
* row r of a chunk equals the rows = 1 call with the draft prefix appended; slot b of a batch equals the batch-1 call;
* neutral parameters are the identity and launch nothing;
* every ValueError of ``LogitProcessor.set``, ``LogitProcessor.__call__``, ``TokenHistory.append`` and ``logprobs`` comes before
  any simulator call;
* the plain loop ``proc(logits, history) -> sampler(logits) -> history.append(result)`` and ``speculative.decode_step(...,
  processor=)`` emit equal tokens, counters and histories, greedy and sampled slots, and the processor adds no copy to the host;
* the fixture of tests/test_gpu_generate_controls.py has what that test needs of it.

Every test but the reference's own hand-worked row names npm_logits_process, npm_history_append, npm_logprob_rows, TokenHistory,
LogitProcessor or logprobs: none of those passes on the parent commit.
"""

import math

import numpy as np
import pytest

import controls_cases as GC
from hostsim.fixtures import npm_fixture
import logits_cases as LC
import logits_reference as LR
import spec_cases as XC


npm = npm_fixture('logits')


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def test_reference_on_a_hand_worked_row():
    z = np.array([2.0, -2.0, 0.5, 1.0, 3.0, -1.0], dtype=np.float32)
    # history 0 0 1 | 3 3 0 with a prompt of 3: seen {0, 1, 3}, counts 0: 1, 3: 2; bias on 2 and 3; eos 4 banned (gen 3 < 5)
    done = LR.process_row(z, [0, 0, 1, 3, 3, 0, 9, -1], 3, 3, 2.0, 0.25, 0.5, 4, 5, [(2, 1.0), (3, -0.5), (2, 7.0), (6, 1.0)], 6)
    assert done == {0, 1, 2, 3, 4}
    assert z.tolist() == [2.0 / 2 - 0.5 - 0.25, -4.0, 1.5, 1.0 / 2 - 1.0 - 0.25 - 0.5, -np.inf, -1.0]
    z = np.array([2.0, -2.0], dtype=np.float32)
    assert LR.process_row(z, [0, 1], 0, 0, 1.0, 0.0, 0.0, 1, 0, [], 2) == set() and z.tolist() == [2.0, -2.0]       # neutral


@pytest.mark.parametrize('name', sorted(LC.CASES))
def test_cases_on_the_simulator_through_the_c_abi(npm, name):
    case = LC.CASES[name]()
    got = LC.check(case)
    want, written = LC.expected(case)
    live = LC.live_slots(case)
    if name not in ('length-0', 'minimum-length'):
        assert written.any(), 'the case changes nothing'
    for b in range(case['batch']):                      # an inactive slot keeps its NaN rows
        if b not in live:
            assert (LC.body(case, got)[b * case['rows']:(b + 1) * case['rows']] == LC.NAN_BITS).all()


@pytest.mark.parametrize('name', ['shapes-V63', 'drafts-rows4', 'drafts-rows8', 'bias-lists', 'minimum-length', 'clipped-lengths'])
def test_a_slot_is_the_batch_one_call_and_a_row_the_one_row_call_with_the_draft_prefix_appended(npm, name):
    case = LC.CASES[name]()
    whole, _ = LC.expected(case)
    rows = case['rows']
    for b in LC.live_slots(case):
        alone = LC.slot_of(case, b)
        assert np.array_equal(LC.body(alone, LC.expected(alone)[0]), LC.body(case, whole)[b * rows:(b + 1) * rows])
        assert np.array_equal(LC.body(alone, LC.run(alone)), LC.body(case, whole)[b * rows:(b + 1) * rows])
        for r in range(min(int(case['n_draft'][b]), rows - 1) + 1):
            single = LC.row_of(case, b, r)
            assert np.array_equal(LC.body(single, LC.run(single))[0], LC.body(case, whole)[b * rows + r]), (b, r)


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def _processor(npm, batch=2, vocab=10, max_bias=3):
    return npm.sampling.LogitProcessor(batch, vocab, max_bias=max_bias)


def test_neutral_parameters_are_the_identity_and_launch_nothing(npm):
    from np_modeling_amd import device as D
    proc = _processor(npm)
    history = npm.sampling.TokenHistory(2, 8)
    history.admit(0, [1, 2, 3])
    host = np.random.default_rng(0).standard_normal([2, 10]).astype(np.float32)
    logits = D.from_host(host)
    before = len(npm.sim.calls), len(npm.sim.d2h)
    assert proc(logits, history) is logits
    proc.set(1, eos=3, min_new_tokens=0)                 # still neutral: the rule can never apply
    proc.set(0, repetition_penalty=1.0, eos=10, min_new_tokens=5)
    assert proc(logits, history, active=[1, 0]) is logits
    assert (len(npm.sim.calls), len(npm.sim.d2h)) == before and 'npm_logits_process' not in npm.sim.calls
    assert np.array_equal(logits.numpy().view(np.uint32), host.view(np.uint32))
    # a neutral slot beside a busy one: only the busy one changes
    proc.set(0, repetition_penalty=2.0)
    proc(logits, history)
    assert npm.sim.calls.count('npm_logits_process') == 1 and npm.sim.npm_last_logits_kernel() == b'hostsim npm_logits_process'
    after = logits.numpy()
    assert np.array_equal(after[1], host[1]) and (after[0, [1, 2, 3]] != host[0, [1, 2, 3]]).all()
    assert np.array_equal(np.delete(after[0], [1, 2, 3]), np.delete(host[0], [1, 2, 3]))
    proc(logits, history)                                # twice applies twice
    assert np.array_equal(logits.numpy()[0, 1], np.float32(host[0, 1] / 4 if host[0, 1] > 0 else host[0, 1] * 4))


def test_the_processor_equals_the_reference_through_the_python_layer(npm):
    from np_modeling_amd import device as D
    proc = _processor(npm, batch=3, vocab=12, max_bias=3)
    proc.set(0, repetition_penalty=1.3, presence_penalty=0.7, frequency_penalty=0.1, logit_bias={5: -math.inf, 2: 0.5}, eos=7,
             min_new_tokens=3, prompt_length=2)
    proc.set(2, frequency_penalty=-0.25, logit_bias=[(11, 1.5)])
    history = npm.sampling.TokenHistory(3, 6)
    for b, ids in enumerate(([4, 4, 7, 4], [1], [3, 3])):
        history.admit(b, ids)
    host = np.random.default_rng(1).standard_normal([3, 12]).astype(np.float32)
    want = host.copy()
    LR.process(want, 3, 1, 12, history=history.numpy(), history_len=[4, 1, 2], history_cap=6, prompt_len=[2, 0, 0],
               repetition=[1.3, 1, 1], presence=[0.7, 0, 0], frequency=[0.1, 0, -0.25], eos=[7, -1, -1], min_new=[3, 0, 0],
               bias_index=[[5, 2, -1], [-1] * 3, [11, -1, -1]], bias_value=[[-np.inf, 0.5, 0], [0] * 3, [1.5, 0, 0]],
               bias_count=[2, 0, 1], bias_cap=3)
    uploads = npm.sim.calls.count('npm_h2d') if 'npm_h2d' in npm.sim.calls else None
    got = proc(D.from_host(host), history).numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and got[0, 5] == -np.inf and got[0, 7] == -np.inf
    assert not proc._stale and uploads is None
    device = proc._device
    proc(D.from_host(host), history)
    assert proc._device is device and not proc._stale                   # one upload after a set, none after that


def test_every_value_error_comes_before_any_simulator_call(npm):
    from np_modeling_amd import device as D
    for bad in (dict(batch=0), dict(vocab=0), dict(vocab=(1 << 20) + 1), dict(max_bias=-1), dict(max_bias=257)):
        with pytest.raises(ValueError):
            npm.sampling.LogitProcessor(**{**dict(batch=2, vocab=10), **bad})
    for bad in ((0, 4), (2, 0)):
        with pytest.raises(ValueError):
            npm.sampling.TokenHistory(*bad)
    proc = _processor(npm)
    history = npm.sampling.TokenHistory(2, 3)
    history.admit(0, [1, 2])
    history.admit(1, [1, 2, 3])
    logits, chunk = D.zeros([2, 10]), D.zeros([6, 10])
    result = npm.sampling.Sampler(2)(D.from_host(np.eye(2, 10, dtype=np.float32)))
    result.numpy()
    snapshot = lambda: tuple(a.copy() for a in (proc.repetition, proc.presence, proc.frequency, proc.eos, proc.min_new, proc.prompt_len,
                                                proc.bias_count, proc.bias_index, proc.bias_value))
    state = snapshot()
    before = len(npm.sim.calls), len(npm.sim.d2h)
    nan, inf = math.nan, math.inf
    for bad in (dict(b=2), dict(b=True), dict(b=-1), dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=inf),
                dict(repetition_penalty=nan), dict(repetition_penalty='1'), dict(presence_penalty=inf), dict(presence_penalty=nan),
                dict(frequency_penalty=-inf), dict(frequency_penalty=None), dict(frequency_penalty=1e39), dict(logit_bias={10: 1.0}),
                dict(logit_bias={-1: 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={1: nan}), dict(logit_bias={1: inf}),
                dict(logit_bias={1: 1e39}), dict(logit_bias=[(1, 0.5), (1, 0.25)]), dict(logit_bias={0: 1, 1: 1, 2: 1, 3: 1}),
                dict(logit_bias=5), dict(logit_bias=[1, 2]), dict(eos=2 ** 31), dict(eos=1.0), dict(min_new_tokens=2 ** 31),
                dict(min_new_tokens=1.5), dict(prompt_length=-2 ** 31 - 1), dict(prompt_length=True)):
        with pytest.raises(ValueError):
            proc.set(**{**dict(b=0), **bad})
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(state, snapshot())), bad
    proc.set(0, repetition_penalty=1.5, logit_bias={1: -inf})
    calls = [lambda: proc(np.zeros([2, 10], dtype=np.float32), history), lambda: proc(D.zeros([2, 9]), history),
             lambda: proc(D.zeros([3, 10]), history), lambda: proc(D.zeros([2 * 65, 10]), history, draft=np.zeros([2, 64], dtype=int), n_draft=[0, 0]),
             lambda: proc(logits, npm.sampling.TokenHistory), lambda: proc(logits, [1, 2]), lambda: proc(chunk, history),
             lambda: proc(chunk, history, draft=np.zeros([2, 2], dtype=int)), lambda: proc(chunk, history, n_draft=[0, 0]),
             lambda: proc(chunk, history, draft=np.zeros([2, 1], dtype=int), n_draft=[0, 0]),
             lambda: proc(chunk, history, draft=np.zeros([2, 2], dtype=int), n_draft=[0, 3]),
             lambda: proc(chunk, history, draft=np.zeros([2, 2], dtype=int), n_draft=[0.0, 1.0]),
             lambda: proc(chunk, history, draft=np.zeros([2, 2], dtype=int), n_draft=[0]),
             lambda: proc(chunk, history, draft=np.zeros([2, 2]), n_draft=[0, 1]),
             lambda: proc(chunk, history, draft=np.zeros([3, 2], dtype=int), n_draft=[0, 1]),
             lambda: proc(chunk, history, draft=np.zeros([2, 2], dtype=int), n_draft=[0, 1], draft_pitch=1),
             lambda: proc(logits, history, active=[1]), lambda: proc(logits, history, active=[1.0, 0.0]),
             lambda: history.append(result), lambda: history.append([1, 2]),
             lambda: history.append(D.IdBuffer([3])), lambda: history.append(result, active=[1]),
             lambda: history.append(result, active=[0.5, 1.0]),
             lambda: npm.sampling.logprobs(np.zeros([2, 10], dtype=np.float32)), lambda: npm.sampling.logprobs(logits, top_n=65),
             lambda: npm.sampling.logprobs(logits, top_n=-1), lambda: npm.sampling.logprobs(logits, top_n=1.0),
             lambda: npm.sampling.logprobs(logits, ids=D.IdBuffer([3]))]
    before = len(npm.sim.calls), len(npm.sim.d2h)
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert (len(npm.sim.calls), len(npm.sim.d2h)) == before, i
    with pytest.raises(ValueError, match='capacity'):      # a bare IdBuffer: its 4 bytes per slot are read to judge the room, nothing more
        history.append(result.ids)
    assert (len(npm.sim.calls), len(npm.sim.d2h)) == (before[0], before[1] + 1) and npm.sim.d2h[-1] == 8
    assert 'npm_logits_process' not in npm.sim.calls and 'npm_history_append' not in npm.sim.calls
    assert 'npm_logprob_rows' not in npm.sim.calls and history.lengths.tolist() == [2, 3]


def test_token_history_appends_on_the_device_and_the_drafter_is_one(npm):
    from np_modeling_amd import device as D
    S = npm.sampling
    assert issubclass(S.NgramDrafter, S.TokenHistory)
    for history in (S.TokenHistory(3, 4), S.NgramDrafter(3, 4, 2)):
        history.admit(0, [5, 6])
        history.admit(2, [7, 7, 7])
        sampler = S.Sampler(3)
        z = np.full([3, 9], -1.0, dtype=np.float32)
        z[0, 4], z[1, 2], z[2, 8] = 1, np.nan, 1               # slot 1 is invalid: token -1
        result = sampler(D.from_host(z))
        copies = len(npm.sim.d2h)
        assert result.numpy().tolist() == [4, -1, 8]
        if isinstance(history, S.NgramDrafter):
            history._ahead = ['stale']
        history.append(result)
        assert len(npm.sim.d2h) == copies + 1 and history._ahead is None       # the result's own copy, cached
        assert history.lengths.tolist() == [3, 0, 4] == history.device_lengths().tolist()
        assert history.numpy()[0, :3].tolist() == [5, 6, 4] and history.numpy()[2].tolist() == [7, 7, 7, 8]
        history.append(result.ids, active=[1, 1, 0])             # a bare IdBuffer: one copy of 4 bytes per slot
        assert npm.sim.d2h[-3:][0] == 12 or 12 in npm.sim.d2h[copies + 1:]
        assert history.lengths.tolist() == [4, 0, 4] == history.device_lengths().tolist() and history.numpy()[0].tolist() == [5, 6, 4, 4]
        with pytest.raises(ValueError, match='capacity'):
            history.append(result)
        history.append(result, active=[0, 1, 0])                 # nothing fits, nothing is asked to
        history.release(0)
        assert history.lengths.tolist() == [0, 0, 4] == history.device_lengths().tolist()
    assert npm.sim.npm_last_logits_kernel() == b'hostsim npm_history_append'


def test_logprobs_on_the_simulator(npm):
    from np_modeling_amd import device as D
    rng = np.random.default_rng(5)
    z = rng.standard_normal([4, 20]).astype(np.float32)
    z[1, 3:9] = -np.inf
    z[2, 0] = np.nan
    ids = np.array([7, 4, 1, -1])
    copies = len(npm.sim.d2h)
    out = npm.sampling.logprobs(D.from_host(z), ids=ids, top_n=5)
    assert len(npm.sim.d2h) == copies
    lse, chosen, tokens, top = out.lse, out.chosen, out.top_tokens, out.top_logprobs
    assert len(npm.sim.d2h) == copies + 1                       # one copy for all four
    for r in (0, 1):
        model = LR.model_logprobs(z[r])
        assert abs(lse[r] - LR.model_lse(z[r])) <= LR.eps(lse[r], 20)
        assert tokens[r].tolist() == np.argsort(-z[r], kind='stable')[:5].tolist()
        assert (np.abs(top[r] - model[tokens[r]]) <= LR.eps(model[tokens[r]], 20)).all()
        assert chosen[r] == -np.inf if z[r, ids[r]] == -np.inf else abs(chosen[r] - model[ids[r]]) <= LR.eps(model[ids[r]], 20)
    assert chosen[1] == -np.inf
    for r in (2, 3):
        assert np.isnan(lse[r]) and np.isnan(chosen[r]) and (tokens[r] == -1).all() and (top[r] == -np.inf).all()
    bare = npm.sampling.logprobs(D.from_host(z))
    assert bare.chosen is None and bare.top_tokens.shape == (4, 0) and np.array_equal(bare.lse[:2], lse[:2]) and not np.isnan(bare.lse[3])
    greedy = npm.sampling.Sampler(4)(D.from_host(z), active=[1, 1, 0, 0])
    out = npm.sampling.logprobs(D.from_host(z), ids=greedy.ids, top_n=1)
    assert np.array_equal(out.chosen[:2].view(np.uint32), out.top_logprobs[:2, 0].view(np.uint32)) and np.isnan(out.chosen[2:]).all()


# ---- speculation stays exact -------------------------------------------------------------------------------------------------------------
def _controls(npm, sampled):
    proc = GC.processor(npm)
    sampler = npm.sampling.Sampler(3)
    if sampled:
        sampler.set(0, temperature=0.9, top_k=12, top_p=0.95, seed=31)
        sampler.set(2, temperature=1.2, top_k=0, top_p=0.8, seed=2 ** 63 + 5)
    return proc, sampler


@pytest.mark.parametrize('sampled', [False, True], ids=['greedy', 'sampled'])
def test_the_speculative_loop_with_a_processor_emits_the_tokens_of_the_plain_loop(npm, sampled):
    model = XC.make_model(npm, seed=GC.SEED)
    proc, sampler = _controls(npm, sampled)
    want, logits, history = GC.plain(npm, model, sampler, proc)
    proc, sampler2 = _controls(npm, sampled)
    calls = npm.sim.calls.count('npm_logits_process')
    got, log, state, drafter = GC.speculative(npm, model, sampler2, proc)
    assert npm.sim.calls.count('npm_logits_process') == calls + 1 + len(log)         # the first token, then one launch a step
    assert [g[:GC.EMIT] for g in got] == want
    accepted, rejected = XC.accepts_and_rejects(log)
    assert accepted >= 1 and rejected >= 1
    emitted = np.array([len(g) for g in got])
    assert sampler2.draw.tolist() == emitted.tolist() == sampler2.device_draw().tolist()
    assert drafter.device_lengths().tolist() == (np.array(XC.PROMPT_LENGTHS) + emitted).tolist() == drafter.lengths.tolist()
    for b in range(3):
        line = drafter.numpy()[b, :drafter.lengths[b]].tolist()
        assert line == model[4][b] + got[b] and line[:XC.PROMPT_LENGTHS[b] + GC.EMIT] == history.numpy()[b, :history.lengths[b]].tolist()
    assert GC.BANNED not in got[1] and GC.EOS not in got[2][:GC.MIN_NEW]
    if not sampled:
        assert GC.least_gap(logits) >= GC.GAP_HOST, 'the seed of tests/test_gpu_generate_controls.py has a near-tie'
        bare, _, _ = GC.plain(npm, model, npm.sampling.Sampler(3), None)
        assert GC.BANNED in bare[1] and GC.EOS in bare[2][:GC.MIN_NEW], 'the ban or the minimum length changes nothing'
        assert GC.EOS in want[2][GC.MIN_NEW:], 'eos never appears once it may'
        flat = [t for g in want for t in g]
        assert len(set(flat)) < len(flat), 'no token repeats: the penalties change nothing'


def test_a_processor_adds_no_copy_to_the_host(npm):
    model = XC.make_model(npm, seed=GC.SEED)
    runs = {}
    for name, proc in (('with', GC.processor(npm)), ('without', None)):
        sampler = npm.sampling.Sampler(3)
        tokens, log, _, _ = GC.speculative(npm, model, sampler, proc, probe=lambda: len(npm.sim.d2h))
        runs[name] = [entry[2] for entry in log]
        assert all(1 <= copies <= 2 for copies in runs[name])
    # the same number of copies per step wherever both runs ran the same kind of step (same slots active, same limits): the
    # processor itself never copies, so the totals may differ only through what the tokens made the drafter do
    proc = GC.processor(npm)
    sampler = npm.sampling.Sampler(3)
    counted = []
    original = proc.__class__.__call__

    def counting(self, *args, **kwargs):
        before = len(npm.sim.d2h)
        out = original(self, *args, **kwargs)
        counted.append(len(npm.sim.d2h) - before)
        return out

    proc.__class__.__call__ = counting
    try:
        GC.speculative(npm, model, sampler, proc)
    finally:
        proc.__class__.__call__ = original
    assert counted and set(counted) == {0}
    assert min(runs['with']) == min(runs['without']) == 1
    # a processor that launches but decides nothing (a bias of 0.0): the very same run, copy for copy
    idle = npm.sampling.LogitProcessor(3, XC.VOCAB, max_bias=1)
    for b in range(3):
        idle.set(b, logit_bias={b: 0.0})
    assert not idle.neutral()
    launches = npm.sim.calls.count('npm_logits_process')
    tokens, log, _, _ = GC.speculative(npm, model, npm.sampling.Sampler(3), idle, probe=lambda: len(npm.sim.d2h))
    bare, bare_log, _, _ = GC.speculative(npm, model, npm.sampling.Sampler(3), None, probe=lambda: len(npm.sim.d2h))
    assert tokens == bare and [entry[2] for entry in log] == [entry[2] for entry in bare_log]
    assert npm.sim.calls.count('npm_logits_process') == launches + 1 + len(log)


def test_decode_step_without_a_processor_makes_the_calls_it_made_before(npm):
    model = XC.make_model(npm, seed=GC.SEED)
    XC.speculative(npm, model, npm.sampling.Sampler(3))                  # the loop of tests/test_spec_host.py: no processor anywhere
    assert 'npm_logits_process' not in npm.sim.calls and 'npm_history_append' not in npm.sim.calls
    assert 'npm_logprob_rows' not in npm.sim.calls


# ---- header against bindings ---------------------------------------------------------------------------------------------------------------
def test_logits_header_bindings_and_struct_layouts():
    import ctypes
    import os
    import re
    import subprocess
    import tempfile
    from np_modeling_amd import _C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'npm_hip.h')).read()
    for struct, mirror in (('npm_logits', _C.npm_logits), ('npm_logprob', _C.npm_logprob)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), text, flags=re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        names = [n.strip().lstrip('*') for decl in body.split(';') if decl.strip()
                 for n in re.sub(r'^\s*(const\s+)?(float|int32_t|int64_t)\s*\*?', '', decl.strip()).split(',')]
        assert names == [f[0] for f in mirror._fields_], struct
    assert int(re.search(r'#define NPM_LOGITS_MAX_BIAS (\d+)', text).group(1)) == _C.LOGITS_MAX_BIAS
    proto = re.search(r'int npm_history_append\((.*?)\);', text, flags=re.S).group(1)
    kinds = [_C._P if '*' in arg else {'int64_t': _C._I64, 'int32_t': _C._I32}[arg.split()[0]] for arg in proto.split(',')]
    assert kinds == _C.SIGNATURES['npm_history_append']
    assert _C.SIGNATURES['npm_logits_process'] == [ctypes.POINTER(_C.npm_logits)]
    assert _C.SIGNATURES['npm_logprob_rows'] == [ctypes.POINTER(_C.npm_logprob)]
    assert _C._SPECIAL['npm_last_logits_kernel'] == (ctypes.c_char_p, [])
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "npm_hip.h"\n'
            'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(npm_logits), offsetof(npm_logits, history), '
            'offsetof(npm_logits, bias_cap), offsetof(npm_logits, workspace), sizeof(npm_logprob), offsetof(npm_logprob, ids), '
            'offsetof(npm_logprob, top_logprob)); return 0;}\n')
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, 'layout.c'), os.path.join(tmp, 'layout')
        open(src, 'w').write(prog)
        subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(root, 'include'), src, '-o', exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_C.npm_logits), _C.npm_logits.history.offset, _C.npm_logits.bias_cap.offset, _C.npm_logits.workspace.offset,
                   ctypes.sizeof(_C.npm_logprob), _C.npm_logprob.ids.offset, _C.npm_logprob.top_logprob.offset]
