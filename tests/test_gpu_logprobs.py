"""GPU: npm_logprob_rows through the C ABI, and ``sampling.logprobs``.

Bounds.  Exact rows ({c, -200, -inf}: tests/sample_cases.py, W1 = m 2^32 whatever the exponential's last bit) are bitwise the
integer model of tests/logits_reference.py: lse, chosen and the top lists; every value is first asserted to lie at least
2^-45 |s| from an fp32 rounding boundary (``beam_cases._off_boundary``), since the device's fp64 log and NumPy's may differ in the
last bit.  General rows lie within ``beam_reference.eps`` of the fp64 log-softmax -- the bound tests/test_gpu_beam.py derives for
the very same expression -- and their top tokens, which depend on the logits' order alone, EQUAL the sorted order.  Against
npm_beam_step everything is bitwise: it is the same kernel.

Every test here needs npm_logprob_rows or ``sampling.logprobs``: none passes on the parent commit.
"""

import ctypes as C

import numpy as np
import pytest

import beam_cases as BC
import logits_reference as LR
import sample_cases as SC
import sample_reference as SR

pytestmark = pytest.mark.gpu

GUARD, S32 = SC.GUARD, SC.SENTINEL32
LAYOUTS = dict(vec=lambda v: dict(pitch=v + (-v) % 4, offset=0), scalar=lambda v: dict(pitch=v + (-v) % 4 + 1, offset=1))


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


def run(z, ids, top_n, pitch=None, offset=0, expect=0):
    """One npm_logprob_rows: dict(lse, chosen (bits) [R], top_token, top_logprob (bits) [R, top_n]); every output between guard
    words, which are asserted untouched; the padding columns hold +inf and NaN."""
    from np_modeling_amd import _C, device as D
    z = np.asarray(z, dtype=np.float32)
    rows, vocab = z.shape
    pitch = vocab if pitch is None else pitch
    host = np.full([offset + rows * pitch], np.nan, dtype=np.float32)
    padded = host[offset:].reshape(rows, pitch)
    padded[:, vocab:] = np.where(np.arange(pitch - vocab) % 2 == 0, np.float32(np.inf), np.float32(np.nan))
    padded[:, :vocab] = z
    logits = D.from_host(host)
    sizes = dict(lse=rows, chosen=rows, top_token=rows * top_n, top_logprob=rows * top_n)
    at, words = {}, GUARD
    for name, size in sizes.items():
        at[name] = words
        words += size + GUARD
    out = D.bytes_from_host(np.full([words], S32, dtype=np.uint32))
    ids_dev = None if ids is None else D.bytes_from_host(np.asarray(ids, dtype=np.int32))
    desc = _C.npm_logprob(logits=logits.ptr + 4 * offset, pitch=pitch, rows=rows, vocab=vocab, top_n=top_n,
                          ids=None if ids is None else ids_dev.ptr, **{name: out.ptr + 4 * first for name, first in at.items()})
    assert _C.lib().npm_logprob_rows(C.byref(desc)) == expect
    after = out.numpy().view(np.uint32)
    keep = np.ones([words], dtype=bool)
    got = {}
    for name, size in sizes.items():
        keep[at[name]:at[name] + size] = False
        got[name] = after[at[name]:at[name] + size].copy()
    assert (after[keep] == S32).all(), 'a guard word around lse / chosen / top_token / top_logprob was written'
    if ids is None:
        assert (got['chosen'] == S32).all(), 'chosen was written without ids'
    got['top_token'] = got['top_token'].view(np.int32).reshape(rows, top_n)
    got['top_logprob'] = got['top_logprob'].reshape(rows, top_n)
    return got


def _model(z, ids, top_n, weights):
    rows = [LR.logprob_row(z[r], None if ids is None else int(ids[r]), top_n, weights) for r in range(z.shape[0])]
    return dict(lse=SC.bits([r[0] for r in rows]), chosen=SC.bits([r[1] for r in rows]), top_token=np.array([r[2] for r in rows]),
                top_logprob=np.stack([SC.bits(r[3]) for r in rows]))


def _same_nan(a, b):
    """uint32 arrays of float bits: equal, a NaN matching any NaN."""
    fa, fb = a.view(np.float32), b.view(np.float32)
    return bool(((a == b) | (np.isnan(fa) & np.isnan(fb))).all())


@pytest.mark.parametrize('vocab', [1, 2, 63, 1000, 4099, SC.LDS_ROW, SC.LDS_ROW + 1])
def test_exact_rows_are_bitwise_the_integer_model(npm, vocab):
    from np_modeling_amd import _C
    z = SC.exact_rows(vocab)
    rng = np.random.default_rng(vocab)
    first_c = [int(np.argmax(z[r] == z[r].max())) for r in range(4)]
    masked = [int(np.argmax(z[r] == -np.inf)) for r in range(4)]               # a -inf token where the row has one (else token 0)
    for ids in (first_c, masked, [vocab - 1, vocab, 2 ** 31 - 1, int(rng.integers(0, vocab))]):
        for top_n in (0, 5, 64):
            want = _model(z, ids, top_n, SR.exact_weights)
            values = np.concatenate([want['lse'], want['chosen'], want['top_logprob'].ravel()]).view(np.float32).astype(np.float64)
            for r in range(4):                                                 # the fp64 values before rounding, off every boundary
                zmax, m = np.float64(z[r].max()), int((z[r] == z[r].max()).sum())
                for v in [zmax + np.log(m)] + [(-zmax - np.log(m)) + np.float64(x) for x in np.unique(z[r][z[r] > -np.inf])]:
                    assert BC._off_boundary(v), (vocab, r)
            assert np.isfinite(values[:4]).all()
            for name, layout in LAYOUTS.items():
                got = run(z, ids, top_n, **layout(vocab))
                assert _C.last_beam_kernel() == (f'logprob_rows_kernel {name} R=4 V={vocab} top={top_n} '
                                                 f'row={"lds" if vocab <= SC.LDS_ROW else "global"}')
                assert np.array_equal(got['top_token'], want['top_token']), (vocab, ids, top_n, name)
                for key in ('lse', 'chosen', 'top_logprob'):
                    assert _same_nan(got[key], want[key]), (vocab, ids, top_n, name, key)


def _general(name):
    if name == 'long':
        return (4 * np.random.default_rng(77).standard_normal([1, SC.LDS_ROW + 4099])).astype(np.float32)
    z = SC.general_rows(int(name)).copy()
    z[1, ::37] = -np.inf                                                       # a masked vocabulary in one row
    return z


@pytest.mark.parametrize('name', ['1000', '8195', 'long'])
def test_general_rows_meet_the_fp64_model_and_npm_beam_step_bit_for_bit(npm, name):
    z = _general(name)
    rows, vocab = z.shape
    order = [np.argsort(-(z[r] + np.float32(0)), kind='stable') for r in range(rows)]
    ids = np.array([order[r][3 % vocab] for r in range(rows)])                 # the fourth most probable token: inside top 20
    model = [LR.model_logprobs(z[r]) for r in range(rows)]
    worst = 0.0
    results = {}
    for layout_name, layout in LAYOUTS.items():
        got = results[layout_name] = run(z, ids, 20, **layout(vocab))
        lse, chosen, top = got['lse'].view(np.float32), got['chosen'].view(np.float32), got['top_logprob'].view(np.float32)
        for r in range(rows):
            assert got['top_token'][r].tolist() == order[r][:20].tolist(), (layout_name, r)
            want = np.concatenate([[LR.model_lse(z[r]), model[r][ids[r]]], model[r][order[r][:20]]])
            have = np.concatenate([[lse[r], chosen[r]], top[r]]).astype(np.float64)
            ratio = np.abs(have - want) / LR.eps(want, vocab)
            worst = max(worst, float(ratio.max()))
            assert (ratio <= 1).all(), (layout_name, r, float(ratio.max()))
        assert np.array_equal(got['chosen'], got['top_logprob'][:, 3]), 'a chosen token inside the top n differs from its entry'
    print(f'logprobs V={vocab}: worst |device - model| / eps = {worst:.3f}')
    assert all(np.array_equal(results['vec'][k], results['scalar'][k]) for k in results['vec'])
    # npm_beam_step on the same rows with cum = 0 and width 1: the same lse, and its first candidate is the first top entry
    beam = BC.run(z, np.zeros([rows], dtype=np.float32), rows, 1, -1)
    assert np.array_equal(beam['lse'].view(np.uint32), results['vec']['lse'])
    assert np.array_equal(beam['cand_score'][:, 0].view(np.uint32), results['vec']['top_logprob'][:, 0])
    assert np.array_equal(beam['cand_token'][:, 0], results['vec']['top_token'][:, 0])
    masked = run(z, np.full([rows], 0 if name == 'long' else 37), 0)
    assert masked['top_token'].shape == (rows, 0) and np.array_equal(masked['lse'], results['vec']['lse'])
    if name != 'long':
        assert masked['chosen'].view(np.float32)[1] == -np.inf                  # the log-probability of a -inf token


def test_skipped_and_invalid_rows_give_nan_and_empty_lists_and_the_others_do_not_notice(npm):
    z = SC.general_rows(1000).copy()
    z[1, 500] = np.nan
    z[2, :] = -np.inf
    poisoned = z.copy()
    poisoned[3, :] = np.inf                                                    # never read: ids[3] < 0
    for layout in LAYOUTS.values():
        got = run(poisoned, [5, 5, 5, -1], 7, **layout(1000))
        alone = run(z[:1], [5], 7, **layout(1000))
        for r in (1, 2, 3):
            assert np.isnan(got['lse'].view(np.float32)[r]) and np.isnan(got['chosen'].view(np.float32)[r])
            assert (got['top_token'][r] == -1).all() and (got['top_logprob'].view(np.float32)[r] == -np.inf).all()
        assert all(np.array_equal(got[k][:1], alone[k]) for k in got)
        inf_row = run(np.where(np.arange(1000) == 9, np.float32(np.inf), z[:1]), None, 3, **layout(1000))
        assert np.isnan(inf_row['lse'].view(np.float32)[0]) and (inf_row['top_token'] == -1).all()
    few = np.full([1, 63], -np.inf, dtype=np.float32)                          # fewer finite tokens than top_n: -1 / -inf behind them
    few[0, [4, 60]] = [1.0, 2.0]
    got = run(few, [4], 5)
    assert got['top_token'][0].tolist() == [60, 4, -1, -1, -1] and (got['top_logprob'].view(np.float32)[0, 2:] == -np.inf).all()
    assert got['chosen'][0] == got['top_logprob'][0, 1]


def test_npm_logprob_rows_refuses_bad_arguments_before_any_launch(npm):
    from np_modeling_amd import _C, device as D
    buf = D.zeros([64])
    run(np.zeros([1, 4], dtype=np.float32), None, 0)
    before = _C.last_beam_kernel()
    ok = dict(logits=buf.ptr, pitch=4, rows=2, vocab=4, top_n=2, ids=buf.ptr, lse=buf.ptr, chosen=buf.ptr, top_token=buf.ptr,
              top_logprob=buf.ptr)
    for change in (dict(rows=0), dict(vocab=0), dict(vocab=(1 << 20) + 1), dict(pitch=3), dict(top_n=-1), dict(top_n=65), dict(logits=None),
                   dict(lse=None), dict(chosen=None), dict(top_token=None), dict(top_logprob=None)):
        assert _C.lib().npm_logprob_rows(C.byref(_C.npm_logprob(**{**ok, **change}))) == 10002, change
    assert _C.lib().npm_logprob_rows(None) == 10002 and _C.last_beam_kernel() == before
    assert np.array_equal(buf.numpy(), np.zeros([64], dtype=np.float32))


def test_sampling_logprobs_on_the_device(npm):
    from np_modeling_amd import device as D
    z = SC.general_rows(1000)
    logits = D.from_host(z)
    result = npm.sampling.Sampler(4)(logits, active=[1, 1, 0, 1])                # greedy; slot 2 sits out: id -1
    out = npm.sampling.logprobs(logits, ids=result.ids, top_n=5)
    want = run(z, result.numpy(), 5)
    assert np.array_equal(SC.bits(out.lse), want['lse']) and np.array_equal(SC.bits(out.chosen), want['chosen'])
    assert np.array_equal(out.top_tokens, want['top_token']) and np.array_equal(SC.bits(out.top_logprobs), want['top_logprob'])
    live = [0, 1, 3]
    assert np.array_equal(SC.bits(out.chosen)[live], SC.bits(out.top_logprobs)[live, 0]) and np.isnan(out.chosen[2])
    assert out.top_tokens[live, 0].tolist() == result.numpy()[live].tolist()
    assert npm.sampling.logprobs(logits).chosen is None
