"""GPU: speculative decoding -- npm_verify_rows and npm_ngram_draft through the C ABI, and ``speculative.decode_step`` end to end.

Bounds: none anywhere.
* npm_verify_rows samples a row with the device function npm_sample_rows samples it with, so token, kept and prob (as uint32) of
  a verified row EQUAL those of npm_sample_rows on that row alone with the counter preset to draw + r -- general logits included.
* On exact-weight rows ({c, -200, -inf}: tests/sample_cases.py) tokens, accepted counts, counters and histories equal the integer
  model of tests/spec_reference.py.
* npm_ngram_draft is integers only: chunk and n_new equal the plain loop of tests/spec_reference.py.
* End to end, greedy: the logits of a T + 1 chunk and of single steps agree to the decode tests' 1e-5 (scaled), not bitwise, so
  each run first asserts from the plain loop's own logits that every top-2 gap is at least 1e-3 of max |logit| -- 100 times that
  tolerance -- and then that the speculative tokens EQUAL the plain ones.  tests/test_spec_host.py picked the seed (5e-3 there).
  Sampled runs are compared on the host simulator only: a near-tie inside a sampled cut has no margin to assert.

Every test here needs npm_verify_rows, npm_ngram_draft, ``truncate``, ``NgramDrafter`` or ``speculative``: none passes on the parent
commit.
"""

import ctypes as C
import itertools

import numpy as np
import pytest

import sample_cases as SC
import spec_cases as XC
import spec_reference as XR

pytestmark = pytest.mark.gpu

GUARD = SC.GUARD
S32, S64 = SC.SENTINEL32, SC.SENTINEL64


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


def _guarded(D, values, dtype, sentinel):
    """``values`` on the device between GUARD sentinel words either side; (buffer, address of the first value)."""
    host = np.full([np.asarray(values).size + 2 * GUARD], sentinel, dtype=dtype)
    host[GUARD:-GUARD] = np.asarray(values, dtype=dtype).reshape(-1)
    buf = D.bytes_from_host(host)
    return buf, buf.ptr + GUARD * host.itemsize


def _inside(buf, dtype, sentinel, what):
    host = buf.numpy().view(dtype)
    assert (host[:GUARD] == sentinel).all() and (host[-GUARD:] == sentinel).all(), f'a guard word around {what} was written'
    return host[GUARD:-GUARD].copy()


class Logits:
    """[batch * rows, V] logits on the device with a row pitch (padding columns: +inf / NaN alternately) and ``offset`` floats in
    front (1: a base 4 bytes off 16-byte alignment); ``sample(r, ...)`` is npm_sample_rows on row r of every slot, ``verify(...)``
    npm_verify_rows on all of them."""

    def __init__(self, npm, logits, rows, pitch=None, offset=0):
        from np_modeling_amd import _C, device as D
        self._C, self._D = _C, D
        logits = np.asarray(logits, dtype=np.float32)
        self.rows, self.vocab, self.batch = rows, logits.shape[1], logits.shape[0] // rows
        self.pitch = self.vocab if pitch is None else pitch
        host = np.full([offset + logits.shape[0] * self.pitch], np.nan, dtype=np.float32)
        padded = host[offset:].reshape(logits.shape[0], self.pitch)
        padded[:, self.vocab:] = np.where(np.arange(self.pitch - self.vocab) % 2 == 0, np.float32(np.inf), np.float32(np.nan))
        padded[:, :self.vocab] = logits
        self.device = D.from_host(host)
        self.base = self.device.ptr + 4 * offset

    def _params(self, temperature, top_k, top_p, seed):
        b = self.batch
        vec = lambda v, dtype: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), [b]))
        host = np.concatenate([vec(seed, np.uint64).view(np.uint8), vec(temperature, np.float32).view(np.uint8),
                               vec(top_k, np.int32).view(np.uint8), vec(top_p, np.float32).view(np.uint8)])
        buf = self._D.bytes_from_host(host)
        return buf, dict(seed=buf.ptr, temperature=buf.ptr + 8 * b, top_k=buf.ptr + 12 * b, top_p=buf.ptr + 16 * b)

    def sample(self, r, temperature, top_k, top_p, seed, draw):
        """(token, kept, prob bits) [batch] of row r of every slot, the counters preset to ``draw`` + r (mod 2^64)."""
        b = self.batch
        keep, params = self._params(temperature, top_k, top_p, seed)
        counters = self._D.bytes_from_host(((np.asarray(draw, dtype=np.uint64) + np.uint64(r))).astype(np.uint64))
        out = self._D.bytes_from_host(np.full([3 * b], S32, dtype=np.uint32))
        desc = self._C.npm_sample(logits=self.base + 4 * r * self.pitch, pitch=self.rows * self.pitch, batch=b, vocab=self.vocab,
                                  draw=counters.ptr, active=None, token=out.ptr, kept=out.ptr + 4 * b, prob=out.ptr + 8 * b, **params)
        self._C.check(self._C.lib().npm_sample_rows(C.byref(desc)), 'npm_sample_rows')
        host = out.numpy().view(np.uint32)
        return host[:b].view(np.int32).copy(), host[b:2 * b].view(np.int32).copy(), host[2 * b:].copy()

    def verify(self, temperature, top_k, top_p, seed, draw, draft, n_draft, history=None, cap=0, history_pitch=None, expect=0):
        """One npm_verify_rows; dict(token, kept, prob (bits) [batch, rows], accepted, draw, history, history_len), guards checked.
        ``history``: per slot the tokens so far (a list of lists), in a [batch, cap] array of pitch ``history_pitch``."""
        D, b, rows = self._D, self.batch, self.rows
        keep, params = self._params(temperature, top_k, top_p, seed)
        draws, draw_ptr = _guarded(D, np.broadcast_to(np.asarray(draw, dtype=np.uint64), [b]), np.uint64, S64)
        outs = {name: _guarded(D, np.full([n], S32, dtype=np.uint32), np.uint32, S32)
                for name, n in dict(token=b * rows, kept=b * rows, prob=b * rows, accepted=b).items()}
        draft = np.asarray(draft, dtype=np.int32).reshape(b, rows - 1)
        draft_dev = D.bytes_from_host(draft if draft.size else np.zeros([1], dtype=np.int32))
        n_dev = D.bytes_from_host(np.asarray(n_draft, dtype=np.int32))
        extra = dict(history=None, history_pitch=0, history_len=None, history_cap=0)
        if history is not None:
            history_pitch = cap if history_pitch is None else history_pitch
            lines = np.full([b, history_pitch], S32, dtype=np.uint32).view(np.int32)
            for s, line in enumerate(history):
                lines[s, :len(line)] = line
            hist, hist_ptr = _guarded(D, lines.view(np.uint32), np.uint32, S32)
            lens, lens_ptr = _guarded(D, np.array([len(line) for line in history], dtype=np.int32).view(np.uint32), np.uint32, S32)
            extra = dict(history=hist_ptr, history_pitch=history_pitch, history_len=lens_ptr, history_cap=cap)
        desc = self._C.npm_verify(logits=self.base, pitch=self.pitch, batch=b, rows=rows, vocab=self.vocab, draw=draw_ptr,
                                  draft=draft_dev.ptr, draft_pitch=draft.shape[1], n_draft=n_dev.ptr, **params, **extra,
                                  **{name: ptr for name, (_, ptr) in outs.items()})
        assert self._C.lib().npm_verify_rows(C.byref(desc)) == expect
        got = {name: _inside(buf, np.uint32, S32, name) for name, (buf, _) in outs.items()}
        got = dict(token=got['token'].view(np.int32).reshape(b, rows), kept=got['kept'].view(np.int32).reshape(b, rows),
                   prob=got['prob'].reshape(b, rows), accepted=got['accepted'].view(np.int32), draw=_inside(draws, np.uint64, S64, 'draw'))
        if history is not None:
            got['history'] = _inside(hist, np.uint32, S32, 'history').view(np.int32).reshape(b, history_pitch)
            got['history_len'] = _inside(lens, np.uint32, S32, 'history_len').view(np.int32)
        return got


def _same_bytes(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


# ---- verify equals sample, bit for bit -------------------------------------------------------------------------------------------------
PARAMS = [dict(temperature=0.0, top_k=0, top_p=1.0), dict(temperature=0.8, top_k=10, top_p=1.0),
          dict(temperature=0.8, top_k=0, top_p=0.9), dict(temperature=0.8, top_k=10, top_p=0.9)]


@pytest.mark.parametrize('vocab', [1, 63, 64, 65, 1000, 4099, 32768, 32769])
def test_npm_verify_rows_equals_npm_sample_rows_row_by_row_as_bits(npm, vocab):
    from np_modeling_amd import _C
    rng = np.random.default_rng(3000 + vocab)
    for rows, batch in itertools.product((1, 2, 5, 9), (1, 3)):
        z = (3 * rng.standard_normal([batch * rows, vocab])).astype(np.float32)
        seed = [11, 2 ** 63 + 12, 13][:batch]
        draw = np.array([2 ** 32 - 2 if rows == 5 else 7, 0, 2 ** 64 - 3][:batch], dtype=np.uint64)         # carries into the high word
        layouts = dict(vec=dict(pitch=vocab + (-vocab) % 4), scalar=dict(pitch=vocab + (-vocab) % 4 + 1, offset=1))
        calls = {name: Logits(npm, z, rows, **layout) for name, layout in layouts.items()}
        for (name, call), params in itertools.product(calls.items(), PARAMS):
            want = [call.sample(r, seed=seed, draw=draw, **params) for r in range(rows)]
            tokens = np.stack([w[0] for w in want], axis=1)
            got = call.verify(seed=seed, draw=draw, draft=tokens[:, :rows - 1], n_draft=[rows - 1] * batch, **params)
            where = (vocab, rows, batch, name, params)
            assert _C.last_sample_kernel() == (f'verify_rows_kernel {name} B={batch} rows={rows} V={vocab} '
                                               f'row={"lds" if vocab <= SC.LDS_ROW else "global"} history=0'), where
            assert ((tokens >= 0) & (tokens < vocab)).all() and np.array_equal(got['token'], tokens), where
            assert np.array_equal(got['kept'], np.stack([w[1] for w in want], axis=1)), where
            assert np.array_equal(got['prob'], np.stack([w[2] for w in want], axis=1)), where
            assert got['accepted'].tolist() == [rows - 1] * batch and np.array_equal(got['draw'], draw + np.uint64(rows)), where


# ---- the exact family ------------------------------------------------------------------------------------------------------------------
ROWS = 4
SLOTS = ['match', 'mismatch at 0', 'mismatch in the middle', 'n_draft 0', 'a -1 draft entry', 'an invalid row', 'inactive']


def _exact_case(vocab):
    """Seven slots of four exact rows each, their parameters, and drafts built from what the model samples: one slot per way a
    draft can end.  (logits, params, draft, n_draft, the integer model's answer per slot)."""
    base = SC.exact_rows(vocab)
    rng = np.random.default_rng(vocab)
    b = len(SLOTS)
    z = np.concatenate([base[rng.permutation(4)] for _ in range(b)])
    params = dict(temperature=[1.0, 0.5, 3.0, 1.0, 0.0, 1.0, 1.0], top_k=[0, 5, 0, 2, 0, 0, 0], top_p=[1.0, 0.5, 0.25, 1.0, 1.0, 0.5, 1.0],
                  seed=SC.EXACT_SEEDS + [5, 6, 7], draw=[0, 3, 2 ** 32 - 2, 9, 1, 2, 77])
    z[5 * ROWS + 1, vocab // 2] = np.nan                               # 'an invalid row': row 1 of slot 5
    z[6 * ROWS:] = np.nan                                              # 'inactive': never read
    model = lambda s, drafted, n: XR.verify(z[s * ROWS:(s + 1) * ROWS], params['temperature'][s], params['top_k'][s],
                                            params['top_p'][s], params['seed'][s], params['draw'][s], drafted, n)
    draft, n_draft = np.zeros([b, ROWS - 1], dtype=np.int64), np.full([b], ROWS - 1)
    for s in range(b - 1):                                             # what is sampled when every drafted token is confirmed
        for r in range(ROWS - 1):
            draft[s, r] = max(model(s, draft[s], r)[0][r], 0)
    other = lambda tok: (tok + 1) % vocab
    draft[1, 0], draft[2, 1], draft[4, 1], n_draft[3], n_draft[6] = other(draft[1, 0]), other(draft[2, 1]), -1, 0, -1
    want = [model(s, draft[s], int(n_draft[s])) for s in range(b)]
    return z, params, draft, n_draft, want


@pytest.mark.parametrize('vocab', [63, 1000, SC.LDS_ROW + 1])
def test_npm_verify_rows_on_exact_rows_equals_the_integer_model(npm, vocab):
    z, params, draft, n_draft, want = _exact_case(vocab)
    b = len(SLOTS)
    assert [w[1] for w in want] == [3, 0, 1, 0, 1, 1, 0]                # every way a draft can end, as the slot names say
    history = [[40 + s] * s for s in range(b)]
    call = Logits(npm, z, ROWS)
    got = call.verify(**params, draft=draft, n_draft=n_draft, history=history, cap=12, history_pitch=13)
    for s, (tokens, accepted, counter, kept, prob) in enumerate(want):
        assert got['token'][s].tolist() == tokens and got['accepted'][s] == accepted and int(got['draw'][s]) == counter, SLOTS[s]
        assert got['kept'][s].tolist() == kept and np.array_equal(got['prob'][s], SC.bits(prob)), SLOTS[s]
        emitted = [t for t in tokens[:accepted + 1] if t >= 0] if n_draft[s] >= 0 else []
        assert got['history'][s, :got['history_len'][s]].tolist() == history[s] + emitted, SLOTS[s]
        assert (got['history'][s, got['history_len'][s]:].view(np.uint32) == S32).all(), SLOTS[s]
    assert got['token'][5].tolist() == [draft[5, 0], -1, -1, -1] and got['history_len'][5] == 5 + 1        # the invalid row ends it
    assert got['token'][6].tolist() == [-1] * ROWS and int(got['draw'][6]) == 77 and got['history_len'][6] == 6
    # two launches are equal as bytes; slot b of the batch is slot b alone
    assert _same_bytes(got, call.verify(**params, draft=draft, n_draft=n_draft, history=history, cap=12, history_pitch=13))
    for s in range(b):
        alone = Logits(npm, z[s * ROWS:(s + 1) * ROWS], ROWS).verify(**{k: [v[s]] for k, v in params.items()}, draft=draft[s:s + 1],
                                                                    n_draft=n_draft[s:s + 1], history=history[s:s + 1], cap=12)
        assert all(np.array_equal(alone[k][0], got[k][s]) for k in ('token', 'kept', 'prob', 'accepted', 'draw', 'history_len')), SLOTS[s]
        assert np.array_equal(alone['history'][0], got['history'][s, :12]), SLOTS[s]
    # a history one short of its capacity takes exactly one token
    full = call.verify(**params, draft=draft, n_draft=n_draft, history=[[9] * 11] * b, cap=12, history_pitch=13)
    for s, (tokens, accepted, _, _, _) in enumerate(want):
        emitted = [t for t in tokens[:accepted + 1] if t >= 0] if n_draft[s] >= 0 else []
        assert full['history_len'][s] == 11 + min(len(emitted), 1) and full['history'][s, :11].tolist() == [9] * 11, SLOTS[s]
        assert full['history'][s, 11:12].tolist() == (emitted[:1] or [S32]) and (full['history'][s, 12:].view(np.uint32) == S32).all(), SLOTS[s]
        assert np.array_equal(full['token'][s], got['token'][s])
    # without the optional outputs and the history: the same tokens
    from np_modeling_amd import _C
    assert 'history=1' in _C.last_sample_kernel()
    bare = call.verify(**params, draft=draft, n_draft=n_draft)
    assert np.array_equal(bare['token'], got['token']) and np.array_equal(bare['draw'], got['draw'])


def test_npm_verify_rows_refuses_bad_arguments_before_any_launch(npm):
    from np_modeling_amd import _C, device as D
    buf = D.zeros([256])
    ok = dict(logits=buf.ptr, pitch=4, batch=2, rows=2, vocab=4, history_cap=4, temperature=buf.ptr, top_k=buf.ptr, top_p=buf.ptr,
              seed=buf.ptr, draw=buf.ptr, draft=buf.ptr, draft_pitch=1, n_draft=buf.ptr, token=buf.ptr, accepted=buf.ptr,
              history=buf.ptr, history_pitch=4, history_len=buf.ptr)
    before = _C.last_sample_kernel()
    for change in (dict(batch=0), dict(rows=0), dict(rows=65), dict(vocab=0), dict(vocab=(1 << 20) + 1), dict(pitch=3), dict(logits=None),
                   dict(draw=None), dict(n_draft=None), dict(token=None), dict(accepted=None), dict(draft=None), dict(draft_pitch=0),
                   dict(history_len=None), dict(history_cap=0), dict(history_pitch=3)):
        assert _C.lib().npm_verify_rows(C.byref(_C.npm_verify(**{**ok, **change}))) == 10002, change
    assert _C.lib().npm_verify_rows(None) == 10002 and _C.last_sample_kernel() == before
    assert np.array_equal(buf.numpy(), np.zeros([256], dtype=np.float32))


# ---- npm_ngram_draft -------------------------------------------------------------------------------------------------------------------
def _draft(npm, histories, limits, t, ngram, cap, pitch):
    from np_modeling_amd import _C, device as D
    b = len(histories)
    lines = np.full([b, pitch], -7, dtype=np.int32)
    for s, line in enumerate(histories):
        lines[s, :len(line)] = line
    hist, lens = D.bytes_from_host(lines), D.bytes_from_host(np.array([len(line) for line in histories], dtype=np.int32))
    lim = D.bytes_from_host(np.asarray(limits, dtype=np.int32))
    chunk, chunk_ptr = _guarded(D, np.full([b * (t + 1)], S32, dtype=np.uint32), np.uint32, S32)
    n_new, n_ptr = _guarded(D, np.full([b], S32, dtype=np.uint32), np.uint32, S32)
    _C.check(_C.lib().npm_ngram_draft(hist.ptr, pitch, cap, lens.ptr, lim.ptr, b, t, ngram[0], ngram[1], chunk_ptr, n_ptr), 'npm_ngram_draft')
    assert _C.last_draft_kernel() == f'ngram_draft_kernel B={b} T={t} ngram={ngram[0]}..{ngram[1]} cap={cap}'
    assert np.array_equal(hist.numpy(), lines.view(np.uint8).reshape(-1))
    return (_inside(chunk, np.uint32, S32, 'chunk').view(np.int32).reshape(b, t + 1), _inside(n_new, np.uint32, S32, 'n_new').view(np.int32))


def test_npm_ngram_draft_on_the_hand_worked_histories(npm):
    for name, (history, t, limit, ngram, (_, _, m), chunk) in sorted(XC.HAND.items()):
        got, n_new = _draft(npm, [history, [], history], [limit, t, limit], t, ngram, cap=16, pitch=16)
        assert got.tolist() == [chunk, [-1] * (t + 1), chunk], name
        assert n_new.tolist() == [0 if not history or limit < 0 else 1 + m, 0] + [0 if not history or limit < 0 else 1 + m], name


@pytest.mark.parametrize('ngram', [(3, 1), (8, 2)], ids=['3-1', '8-2'])
@pytest.mark.parametrize('t', [1, 4, 7])
def test_npm_ngram_draft_on_random_histories_equals_the_plain_loop(npm, t, ngram):
    """A 4-token alphabet that holds the ids 0 and 2^31 - 1, so that matches abound; every length around the block size and the
    n-gram sizes with every limit, one slot each, in a history array whose pitch exceeds its capacity."""
    rng = np.random.default_rng(100 * t + ngram[0])
    alphabet = np.array([0, 5, 17, 2 ** 31 - 1])
    lengths = [0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1025, 4097]
    histories, limits = [], []
    for length in lengths:
        line = alphabet[rng.integers(0, 4, size=length)].tolist()
        for limit in (-1, 0, 2, t):
            histories.append(line)
            limits.append(limit)
    got, n_new = _draft(npm, histories, limits, t, ngram, cap=4097, pitch=4100)
    found = set()
    for s, (line, limit) in enumerate(zip(histories, limits)):
        chunk, count, (n, j, m) = XR.draft(line, t, limit, *ngram)
        assert got[s].tolist() == chunk and n_new[s] == count, (len(line), limit, n, j, m)
        found.add(n)
    assert len(found - {None}) >= 2 and None in found                   # several n-gram sizes decided, and no match at all
    with_limit_null = XR.draft(histories[-1], t, t, *ngram)[0]
    from np_modeling_amd import _C, device as D
    hist = D.bytes_from_host(np.asarray(histories[-1], dtype=np.int32))
    out = D.bytes_from_host(np.full([t + 2], S32, dtype=np.uint32))
    lens = D.bytes_from_host(np.array([4097], dtype=np.int32))
    _C.check(_C.lib().npm_ngram_draft(hist.ptr, 4097, 4097, lens.ptr, None, 1, t, ngram[0], ngram[1], out.ptr, out.ptr + 4 * (t + 1)),
             'npm_ngram_draft')
    assert out.numpy().view(np.int32)[:t + 1].tolist() == with_limit_null                                  # limit NULL: T
    ok = dict(history=hist.ptr, history_pitch=4097, history_cap=4097, history_len=lens.ptr, limit=None, batch=1, max_draft=t,
              nmax=3, nmin=1, chunk=out.ptr, n_new=out.ptr)
    for change in (dict(batch=0), dict(max_draft=64), dict(max_draft=-1), dict(nmin=0), dict(nmax=9), dict(nmax=1, nmin=2),
                   dict(history_pitch=4096), dict(history_cap=0), dict(history=None), dict(chunk=None), dict(n_new=None),
                   dict(history_len=None)):
        assert _C.lib().npm_ngram_draft(*{**ok, **change}.values()) == 10002, change


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('setting', [dict(), dict(cache_dtype='f16'), dict(window=8)], ids=['f32', 'f16', 'window8'])
def test_greedy_speculative_decode_step_emits_the_tokens_of_the_one_token_loop(npm, setting):
    model = XC.make_model(npm, window=setting.get('window'))
    dtype = setting.get('cache_dtype', 'f32')
    want, logits, pages, lengths = XC.plain(npm, model, npm.sampling.Sampler(3), cache_dtype=dtype)
    gap = XC.least_gap(logits)
    print(f'speculative {setting}: least top-2 gap of the plain run {gap:.3e} of max |logit|')
    assert gap >= XC.GAP, 'the fixture has a near-tie: chunked and single-step logits may pick different tokens'
    sampler = npm.sampling.Sampler(3)
    got, log, state, drafter = XC.speculative(npm, model, sampler, cache_dtype=dtype)
    accepted, rejected = XC.accepts_and_rejects(log)
    print(f'speculative {setting}: {len(log)} steps for {[len(g) for g in got]} tokens, slot-steps accepting {accepted}, rejecting {rejected}')
    assert [g[:XC.EMIT] for g in got] == want and np.array(want).shape == (3, XC.EMIT)
    assert accepted >= 1 and rejected >= 1 and len(log) < XC.EMIT - 1
    emitted = np.array([len(g) for g in got])
    assert sampler.draw.tolist() == emitted.tolist() == sampler.device_draw().tolist()
    assert drafter.device_lengths().tolist() == (np.array(XC.PROMPT_LENGTHS) + emitted).tolist()
    state.truncate(emitted - XC.EMIT)                                  # stop at the budget: both loops hold the same rows
    assert state.positions.tolist() == lengths.tolist() and state.self_cache.pages_in_use == pages
