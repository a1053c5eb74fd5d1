"""TEST INFRASTRUCTURE ONLY -- the cases of npm_beam_step shared by tests/test_beam_host.py (host simulator) and
tests/test_gpu_beam.py (device): the general family judged against the fp64 model, the exact family judged bitwise against the
contract, a runner that surrounds every output and the workspace with guard words, and the assertions themselves.

General rows: N(0, 1) logits times ``scale`` in {1, 4}, cum uniform in [-3 scale, 0]; from V = 63 on about 3 % of the tokens are
masked with -inf, and from W = 3 on beam 1 of group 0 is dead.  Exact rows: logits over {c, -200, -inf} with m copies of the
maximum, so that W1 = m 2^32 whatever the exponential's last bit, filtered (``exact_ok``) to rows whose fp64 scores and lse lie
at least 2^-45 |s| from an fp32 rounding boundary: the device's fp64 log and NumPy's may differ in the last bit.
"""

import ctypes as C
import functools
import zlib

import numpy as np

import beam_reference as BR
import sample_reference as SR

VOCABS = (1, 2, 63, 64, 65, 255, 1000, 4099, 32767, 32768, 32769, 65537)
WIDTHS = (1, 2, 3, 8, 32)
GROUPS = (1, 3)
SCALES = (1.0, 4.0)
GENERAL = [(v, w, g, s) for v in VOCABS for w in WIDTHS for g in GROUPS for s in SCALES]
GUARD = 0x6B6B6B6B


def general_id(case):
    return 'V%d-W%d-G%d-x%g' % case


@functools.lru_cache(maxsize=2)
def general(vocab, width, groups, scale):
    """(logits [G W, V], cum [G W], eos)."""
    rng = np.random.default_rng(zlib.crc32(repr((vocab, width, groups, scale)).encode()))
    n = groups * width
    logits = (rng.standard_normal([n, vocab]) * scale).astype(np.float32)
    if vocab >= 63:
        logits[rng.random([n, vocab]) < 0.03] = -np.inf
    cum = rng.uniform(-3 * scale, 0, size=n).astype(np.float32)
    if width >= 3:
        cum[1] = -np.inf
    return logits, cum, int(rng.integers(0, min(vocab, 8)))


class Model:
    """The fp64 model of one case: scores [G W, V], per-row lse, the first C + 1 candidates of every group, and whether any gap
    among them is within 2 eps (``ambiguous``: the device's list need not equal the model's)."""

    def __init__(self, logits, cum, groups, width):
        self.vocab = logits.shape[1]
        self.scores = BR.model_scores(logits, cum)
        self.lse = np.array([BR.model_lse(logits[r]) if BR.live(cum[r]) and not SR.invalid_row(logits[r], 1.0, 1.0) else np.nan
                             for r in range(groups * width)])
        self.top = BR.model_top(self.scores, groups, width, 2 * width + 1)
        self.ambiguous = [any(a[0] - b[0] <= 2 * BR.eps(b[0], self.vocab) for a, b in zip(top, top[1:])) for top in self.top]


def exact_rows(seed, vocab, width, groups, copies, constants=(0.0, 1.5, -3.25, 7.0), cums=(0.0, -0.5, -1.25, -2.0), masked=0.2,
               dead=0.0):
    """(logits, cum): every row holds min(copies, V) copies of its maximum c, -200 elsewhere and -inf with probability
    ``masked``; cum from a small set, so that scores tie across beams."""
    rng = np.random.default_rng(seed)
    n = groups * width
    logits = np.full([n, vocab], -200.0, dtype=np.float32)
    logits[rng.random([n, vocab]) < masked] = -np.inf
    for r in range(n):
        logits[r, rng.choice(vocab, size=min(copies, vocab), replace=False)] = rng.choice(constants)
    cum = rng.choice(cums, size=n).astype(np.float32)
    cum[rng.random(n) < dead] = -np.inf
    return logits, cum


def _off_boundary(s64) -> bool:
    """Whether the fp64 value lies at least 2^-45 |s| from the nearest boundary between two fp32 roundings."""
    f = np.float32(s64)
    for other in (np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
        boundary = (np.float64(f) + np.float64(other)) / 2
        if abs(s64 - boundary) < 2.0 ** -45 * abs(s64):
            return False
    return True


def exact_ok(logits, cum, width) -> bool:
    """The filter of the exact family, from the reference alone."""
    import math
    for r in range(logits.shape[0]):
        if not BR.live(cum[r]) or SR.invalid_row(logits[r], 1.0, 1.0):
            continue
        z = logits[r]
        zmax = np.float64(z.max() + np.float32(0))
        n = math.log(float(int(SR.exact_weights(z, 1.0).sum())) * 2.0 ** -32)
        values = [zmax + n] + [((np.float64(cum[r]) - zmax) - n) + np.float64(v) for v in np.unique(z[z > -np.inf])]
        if not all(_off_boundary(v) for v in values):
            return False
    return True


# (name, seed, V, W, G, copies, eos, keyword arguments of exact_rows)
EXACT = [
    ('one-max', 1, 1000, 3, 2, 1, 5, {}),
    ('two-max', 2, 4099, 8, 1, 2, -1, {}),
    ('three-max-global-row', 3, 32769, 2, 3, 3, 7, {}),
    ('seven-max-quota', 4, 65, 1, 3, 7, -1, dict(masked=0.0)),                       # C = 2 of 7 equal keys: the lowest indices
    ('cut-inside-the-ties', 5, 1000, 8, 1, 3, 2, dict(masked=0.0)),                  # 3 maxima, then 13 of 997 equal keys
    ('ties-across-beams', 6, 255, 3, 2, 2, -1, dict(constants=(1.5,), cums=(-0.5,), masked=0.0)),
    ('wide', 7, 32768, 32, 1, 2, 3, dict(dead=0.2)),
    ('single-token', 8, 1, 3, 2, 1, -1, dict(masked=0.0)),
    ('lds-edge-ties', 9, 32767, 3, 1, 7, 0, dict(constants=(0.0,), cums=(0.0, -1.25))),
]


def exact(name):
    """(logits, cum, groups, width, eos) of the named exact case; AssertionError if the filter refuses it."""
    _, seed, vocab, width, groups, copies, eos, kw = next(c for c in EXACT if c[0] == name)
    logits, cum = exact_rows(seed, vocab, width, groups, copies, **kw)
    assert exact_ok(logits, cum, width), name
    return logits, cum, groups, width, eos


# ---- the runner -------------------------------------------------------------------------------------------------------------------
def run(logits, cum, groups, width, eos, pitch=None, offset=0, rows=None):
    """One npm_beam_step through np_modeling_amd._C on whatever library is installed.  ``logits`` [G W, V] goes up with row
    pitch ``pitch`` (NaN between the rows) at ``offset`` floats past a 16-byte aligned base; every output and the workspace sit
    in one buffer between guard words, which are asserted untouched.  ``rows``: what is uploaded in place of ``logits``
    (a test that poisons dead rows).  Returns the seven results as host arrays, ``cum`` being the updated one."""
    from np_modeling_amd import _C
    from np_modeling_amd import device as D
    n, vocab = logits.shape
    assert n == groups * width
    pitch, cands = vocab if pitch is None else pitch, 2 * width
    host = np.full([offset + n * pitch], np.nan, dtype=np.float32)
    for r in range(n):
        host[offset + r * pitch:offset + r * pitch + vocab] = (logits if rows is None else rows)[r]
    dev = D.bytes_from_host(host)
    sizes = [('cum', n), ('parent', n), ('ids', n), ('lse', n), ('cand_slot', groups * cands), ('cand_token', groups * cands),
             ('cand_score', groups * cands), ('workspace', _C.beam_workspace_bytes(groups, width) // 4)]
    at, words = {}, 1
    for name, size in sizes:
        at[name] = words
        words += size + 1
    image = np.full([words], GUARD, dtype=np.uint32)
    image[at['cum']:at['cum'] + n] = np.asarray(cum, dtype=np.float32).view(np.uint32)
    out = D.bytes_from_host(image)
    address = {name: out.ptr + 4 * first for name, first in at.items()}
    desc = _C.npm_beam(logits=dev.ptr + 4 * offset, pitch=pitch, groups=groups, width=width, vocab=vocab, eos=eos,
                       workspace_bytes=4 * sizes[-1][1], **address)
    _C.check(_C.lib().npm_beam_step(C.byref(desc)), 'npm_beam_step')
    after = out.numpy().view(np.uint32)
    result = {}
    for name, size in sizes:
        first = at[name]
        assert after[first - 1] == GUARD and after[first + size] == GUARD, f'a guard word next to {name} was overwritten'
        if name != 'workspace':
            block = after[first:first + size].copy()
            result[name] = block.view(np.float32) if name in ('cum', 'lse', 'cand_score') else block.view(np.int32)
    for name in ('cand_slot', 'cand_token', 'cand_score'):
        result[name] = result[name].reshape(groups, cands)
    return result


def same_bits(a, b) -> bool:
    return all(np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32))
               for k in ('cum', 'parent', 'ids', 'lse', 'cand_slot', 'cand_token', 'cand_score'))


# ---- the assertions ---------------------------------------------------------------------------------------------------------------
def check_split(out, groups, width, eos):
    """(e): parent, ids and cum are exactly what step 9 gives on the device's own candidate list; returns the finished sets."""
    finished = []
    for g in range(groups):
        parent, ids, cum, done = BR.split(out['cand_slot'][g], out['cand_token'][g], out['cand_score'][g], g * width, width, eos)
        rows = slice(g * width, (g + 1) * width)
        assert out['parent'][rows].tolist() == parent and out['ids'][rows].tolist() == ids, (g, out['parent'][rows], parent)
        assert np.array_equal(out['cum'][rows].view(np.uint32), np.array(cum, dtype=np.float32).view(np.uint32)), g
        finished.append(done)
    return finished


def check_general(out, logits, cum, groups, width, eos, model):
    """(a) - (f) of one general case; returns the worst |device - model| / eps over scores and lse."""
    vocab, cands = logits.shape[1], 2 * width
    worst = 0.0
    keys = -(logits + np.float32(0))                                              # ascending keys: the row order of equal scores
    for g in range(groups):
        slot, token, score = out['cand_slot'][g], out['cand_token'][g], out['cand_score'][g]
        block = model.scores[g * width:(g + 1) * width]
        count = min(cands, int((block > -np.inf).sum()))
        assert (slot[count:] == -1).all() and (token[count:] == -1).all() and (score[count:] == -np.inf).all(), (g, count)
        slot, token, score = slot[:count], token[:count], score[:count]
        # (a) distinct, legal, from live and valid rows (a dead, invalid or masked entry has model score -inf)
        assert ((slot >= g * width) & (slot < (g + 1) * width) & (token >= 0) & (token < vocab)).all(), g
        assert len(set(zip(slot.tolist(), token.tolist()))) == count, g
        chosen = model.scores[slot, token]
        assert (chosen > -np.inf).all(), g
        # (b) scores within eps of the model
        ratio = np.abs(score.astype(np.float64) - chosen) / BR.eps(chosen, vocab)
        worst = max(worst, float(ratio.max()) if count else 0.0)
        assert (ratio <= 1).all(), (g, float(ratio.max()))
        # (c) the contract's order by the list's own scores
        for p in range(count - 1):
            a = (-float(score[p]), int(slot[p]), float(keys[slot[p], token[p]]), int(token[p]))
            b = (-float(score[p + 1]), int(slot[p + 1]), float(keys[slot[p + 1], token[p + 1]]), int(token[p + 1]))
            assert a < b, (g, p, a, b)
        # (d) nothing omitted beats the weakest chosen by more than 2 eps
        if count:
            rest = block.copy()
            rest[slot - g * width, token] = -np.inf
            assert rest.max() <= chosen.min() + 2 * BR.eps(chosen.min(), vocab), (g, float(rest.max()), float(chosen.min()))
        if not model.ambiguous[g]:
            assert list(zip(slot.tolist(), token.tolist())) == [(s, t) for _, s, t in model.top[g][:cands]], g
    check_split(out, groups, width, eos)                                          # (e)
    for r in range(groups * width):                                               # (f)
        if np.isnan(model.lse[r]):
            assert np.isnan(out['lse'][r]), r
        else:
            ratio = abs(float(out['lse'][r]) - model.lse[r]) / BR.eps(model.lse[r], vocab)
            worst = max(worst, ratio)
            assert ratio <= 1, (r, ratio)
    return worst


def check_exact(out, logits, cum, groups, width, eos):
    """Bitwise the contract with exact integer weights."""
    want = BR.step(logits, cum, groups, width, eos, weights=BR.exact_weights)
    for k in ('cand_slot', 'cand_token', 'parent', 'ids'):
        assert np.array_equal(out[k], want[k]), (k, out[k], want[k])
    for k in ('cand_score', 'cum', 'lse'):
        assert np.array_equal(out[k].view(np.uint32), want[k].view(np.uint32)), (k, out[k], want[k])
    return want


# ---- edge cases, run by both test files on whatever library is installed ------------------------------------------------------------
def _small(seed, vocab, width, groups):
    rng = np.random.default_rng(seed)
    n = groups * width
    return rng.standard_normal([n, vocab]).astype(np.float32), rng.uniform(-3, 0, size=n).astype(np.float32)


def edge_pitch_and_misaligned_base():
    """A pitch above V (not a multiple of 4 either) and a base one float past alignment: the one-float-per-lane path gives the
    aligned call's bits."""
    from np_modeling_amd import _C
    for vocab in (1000, 32769):
        logits, cum = _small(vocab, vocab, 3, 2)
        plain = run(logits, cum, 2, 3, 4)
        kernel = _C.last_beam_kernel()
        assert 'hostsim' in kernel or ('vec' in kernel) == (vocab % 4 == 0), kernel
        for pitch, offset in ((vocab + 7, 0), (vocab + 4 - vocab % 4, 1), (vocab + 4 - vocab % 4, 0)):
            assert same_bits(run(logits, cum, 2, 3, 4, pitch=pitch, offset=offset), plain), (vocab, pitch, offset)
            kernel = _C.last_beam_kernel()
            assert 'hostsim' in kernel or ('vec' in kernel) == (pitch % 4 == 0 and offset == 0), kernel
        check_general(plain, logits, cum, 2, 3, 4, Model(logits, cum, 2, 3))


def edge_fewer_candidates_than_slots():
    """V = 1, W = 3: one candidate per live beam."""
    logits = np.array([[0.5], [-1.0], [2.0]], dtype=np.float32)
    out = run(logits, np.array([-1.0, -0.25, -2.0], dtype=np.float32), 1, 3, -1)
    assert out['cand_slot'][0].tolist() == [1, 0, 2, -1, -1, -1] and out['cand_token'][0].tolist() == [0, 0, 0, -1, -1, -1]
    assert out['cand_score'][0].tolist() == [-0.25, -1.0, -2.0] + [-np.inf] * 3       # log-softmax of one token is 0
    assert out['parent'].tolist() == [1, 0, 2] and out['ids'].tolist() == [0, 0, 0] and out['lse'].tolist() == [0.5, -1.0, 2.0]
    out = run(logits, np.array([-1.0, -np.inf, -2.0], dtype=np.float32), 1, 3, 0)      # the only token is eos: nothing lives on
    assert out['cand_slot'][0].tolist() == [0, 2, -1, -1, -1, -1] and out['parent'].tolist() == [-1] * 3
    assert check_split(out, 1, 3, 0) == [[0, 1]] and (out['cum'] == -np.inf).all()


def edge_dead_rows_are_not_read():
    """Dead rows filled with NaN give the bits of the same call with those rows zeroed; a cum of NaN is dead too."""
    logits, cum = _small(11, 4099, 3, 3)
    cum[[1, 3, 4, 5]] = [-np.inf, np.nan, -np.inf, -np.inf]                           # group 1 is all dead
    poisoned, zeroed = logits.copy(), logits.copy()
    poisoned[[1, 3, 4, 5]], zeroed[[1, 3, 4, 5]] = np.nan, 0
    a, b = run(logits, cum, 3, 3, 2, rows=poisoned), run(logits, cum, 3, 3, 2, rows=zeroed)
    assert same_bits(a, b)
    assert np.isnan(a['lse'][[1, 3, 4, 5]]).all() and not np.isnan(a['lse'][[0, 2, 6, 7, 8]]).any()
    assert (a['cand_slot'][1] == -1).all() and (a['cand_token'][1] == -1).all() and (a['cand_score'][1] == -np.inf).all()
    assert a['parent'][3:6].tolist() == [-1] * 3 and a['ids'][3:6].tolist() == [-1] * 3 and (a['cum'][3:6] == -np.inf).all()
    assert not (a['cand_slot'] == 1).any()
    live = logits.copy()
    live[[1, 3, 4, 5]] = -np.inf                                                      # the model: those rows offer nothing
    dead_cum = np.where(np.isnan(cum), -np.inf, cum).astype(np.float32)
    check_general(a, live, dead_cum, 3, 3, 2, Model(live, dead_cum, 3, 3))


def edge_a_live_invalid_row_contributes_nothing():
    """A NaN, a +inf or nothing but -inf in a live row: lse NaN, no candidate from it, the other beams as if it were dead."""
    logits, cum = _small(12, 1000, 3, 1)
    dead = cum.copy()
    dead[1] = -np.inf
    want = run(logits, dead, 1, 3, 5)
    for bad in (np.nan, np.inf, None):
        rows = logits.copy()
        if bad is None:
            rows[1] = -np.inf
        else:
            rows[1, 777] = bad
        out = run(rows, cum, 1, 3, 5)
        assert same_bits(out, want), bad
        assert np.isnan(out['lse'][1]) and not (out['cand_slot'] == 1).any()


def edge_eos_positions():
    """eos below position W is finished and the next beams are filled from behind it; at W or above it is ignored; a negative
    eos splits nothing.  Exact rows, so the candidate order is known: W = 2, one live beam with its maxima at tokens 3, 5, 7, 9."""
    logits = np.full([2, 64], -200.0, dtype=np.float32)
    logits[0, [3, 5, 7, 9]] = 1.5
    cum = np.array([-0.5, -np.inf], dtype=np.float32)
    assert exact_ok(logits, cum, 2)
    base = check_exact(run(logits, cum, 1, 2, -1), logits, cum, 1, 2, -1)
    assert base['cand_token'][0].tolist() == [3, 5, 7, 9] and base['ids'].tolist() == [3, 5] and base['finished'] == [[]]
    below = run(logits, cum, 1, 2, 5)
    check_exact(below, logits, cum, 1, 2, 5)
    assert check_split(below, 1, 2, 5) == [[1]] and below['ids'].tolist() == [3, 7] and below['parent'].tolist() == [0, 0]
    first = run(logits, cum, 1, 2, 3)
    assert check_split(first, 1, 2, 3) == [[0]] and first['ids'].tolist() == [5, 7]
    above = run(logits, cum, 1, 2, 7)                                                  # position 2 = W: ignored, never a beam
    check_exact(above, logits, cum, 1, 2, 7)
    assert check_split(above, 1, 2, 7) == [[]] and above['ids'].tolist() == [3, 5]
    for eos in (-1, -7):
        assert same_bits(run(logits, cum, 1, 2, eos), run(logits, cum, 1, 2, 1 << 20))
    for out in (below, first, above):
        for k in ('cand_slot', 'cand_token', 'cand_score', 'lse'):
            assert np.array_equal(out[k].view(np.uint32), np.asarray(base[k]).view(np.uint32)), k    # eos changes the split only


def edge_groups_are_independent_and_launches_repeat():
    """Group g of a batch is bitwise the G = 1 call on that group, and two launches are bitwise equal."""
    for vocab, width in ((4099, 8), (65537, 2)):
        logits, cum = _small(vocab + width, vocab, width, 3)
        cum[width + 1] = -np.inf
        whole = run(logits, cum, 3, width, 1)
        assert same_bits(whole, run(logits, cum, 3, width, 1))
        for g in range(3):
            rows = slice(g * width, (g + 1) * width)
            alone = run(logits[rows], cum[rows], 1, width, 1)
            for k in ('cum', 'ids', 'lse'):
                assert np.array_equal(alone[k].view(np.uint32), whole[k][rows].view(np.uint32)), (g, k)
            assert np.array_equal(np.where(alone['parent'] >= 0, alone['parent'] + g * width, -1), whole['parent'][rows]), g
            assert np.array_equal(np.where(alone['cand_slot'][0] >= 0, alone['cand_slot'][0] + g * width, -1), whole['cand_slot'][g]), g
            for k in ('cand_token', 'cand_score'):
                assert np.array_equal(alone[k][0].view(np.uint32), whole[k][g].view(np.uint32)), (g, k)


def edge_bad_arguments():
    """Every refusal of the entry point, with nothing written."""
    from np_modeling_amd import _C
    from np_modeling_amd import device as D
    logits = D.from_host(np.zeros([4, 8], dtype=np.float32))
    out = D.bytes_from_host(np.full([256], GUARD, dtype=np.uint32))
    good = dict(logits=logits.ptr, pitch=8, groups=2, width=2, vocab=8, eos=-1, cum=out.ptr, parent=out.ptr + 16, ids=out.ptr + 32,
                lse=out.ptr + 48, cand_slot=out.ptr + 64, cand_token=out.ptr + 96, cand_score=out.ptr + 128, workspace=out.ptr + 160,
                workspace_bytes=_C.beam_workspace_bytes(2, 2))
    assert _C.beam_workspace_bytes(2, 2) == 4 * 4 * 9
    bad = [dict(groups=0), dict(width=0), dict(width=33), dict(vocab=0), dict(vocab=(1 << 20) + 1, pitch=1 << 21), dict(pitch=7),
           dict(workspace_bytes=_C.beam_workspace_bytes(2, 2) - 4), dict(workspace=out.ptr + 161)]
    bad += [{name: None} for name in ('logits', 'cum', 'parent', 'ids', 'lse', 'cand_slot', 'cand_token', 'cand_score', 'workspace')]
    for change in bad:
        assert _C.lib().npm_beam_step(C.byref(_C.npm_beam(**{**good, **change}))) == 10002, change
    assert (out.numpy().view(np.uint32) == GUARD).all()
    assert _C.lib().npm_beam_step(None) == 10002


# ---- reorder --------------------------------------------------------------------------------------------------------------------------
ROW = 32                                   # Hkv * D of the bare caches below: 2 heads of 16


def cache_rows(seed, count):
    return np.random.default_rng(seed).standard_normal([count, ROW]).astype(np.float32)


def cache_append(D, cache, new_rows):
    """``new_rows``: per sequence an array [n_b, ROW] or None; one ragged append of the same rows as K and V."""
    n = np.array([0 if r is None else len(r) for r in new_rows], dtype=np.int64)
    t = max(int(n.max()), 1)
    x = np.zeros([cache.batch, t, ROW], dtype=np.float32)
    for b, r in enumerate(new_rows):
        if r is not None:
            x[b, :len(r)] = r
    dev = D.from_host(x)
    cache.append(D.Mat(dev, ROW), D.Mat(dev, ROW), t, new_lengths=n)


def cache_state(cache):
    state = [cache.lengths.copy()]
    if cache.paged:
        state += [cache.block_table.copy(), cache.refcount.copy(), np.array(sorted(cache._free)), cache.dropped.copy()]
    return state


def refcount_is_the_number_of_table_entries(cache):
    named = np.bincount(cache.block_table[cache.block_table >= 0], minlength=cache.pages)
    assert np.array_equal(cache.refcount, named), (cache.refcount, named)
    assert sorted(cache._free) == np.nonzero(named == 0)[0].tolist()


def gathered(cache):
    """The valid rows of every sequence, K (V holds the same): a list of [L_b, ROW]."""
    if not cache.max_length:
        return [np.zeros([0, ROW], dtype=np.float32) for _ in range(cache.batch)]
    k, v = cache.gather(cache.max_length)
    k, v = np.asarray(k).reshape(cache.batch, -1, ROW), np.asarray(v).reshape(cache.batch, -1, ROW)
    assert np.array_equal(k, v)
    return [k[b, :cache.lengths[b]] for b in range(cache.batch)]


def reorder_through_a_spare_slot(cache, parents):
    """``reorder`` written with ``release`` / ``fork`` and slot B - 1 as the spare (it must be empty and no parent)."""
    spare, p = cache.batch - 1, list(parents)
    assert cache.lengths[spare] == 0 and p[spare] == -1 and spare not in p
    done = [b for b in range(spare) if p[b] == b or (p[b] == -1 and cache.lengths[b] == 0)]
    todo = [b for b in range(spare) if b not in done]
    while todo:
        free = [b for b in todo if not any(p[o] == b for o in todo if o != b)]     # nobody still needs what this slot holds
        if free:
            b = free[0]
        else:                                                                      # a cycle: its first slot moves to the spare
            b = todo[0]
            cache.release(spare)                                                       # what an earlier cycle left there is placed by now
            cache.fork(b, spare)
            p = [spare if v == b else v for v in p]
        cache.release(b)
        if p[b] >= 0:
            cache.fork(p[b], b)
        todo.remove(b)
    cache.release(spare)


REORDERS = ([0, 1, 2, 3, -1], [1, 0, 3, 2, -1], [1, 2, 3, 0, -1], [2, 2, 2, 2, -1], [0, 0, 1, -1, -1], [-1, -1, -1, -1, -1],
            [3, 3, 0, 0, -1], [0, 2, 1, 1, -1])


def reorder_paged_equals_release_and_fork(D, **kwargs):
    """Two caches built alike, one reordered, one rearranged through the spare slot: the same table, refcount, lengths, dropped
    and free pages; the same rows gathered; refcount the number of table entries throughout; no launch; an upload only when a
    row changed."""
    caches = [D.PagedKVCache(5, 256, 2, 16, page_size=16, **kwargs) for _ in range(2)]
    for cache in caches:
        cache_append(D, cache, [cache_rows(b, n) for b, n in enumerate((40, 16, 5, 33))] + [None])
    step = 0
    for parents in REORDERS * 2:
        a, b = caches
        rows = gathered(a) if not a.dropped.any() else None
        a._device_table()
        uploads, changed = a.table_uploads, not np.array_equal(np.where(np.array(parents)[:, None] >= 0, a.block_table[parents], -1),
                                                               a.block_table)
        a.reorder(parents)
        reorder_through_a_spare_slot(b, parents)
        for x, y in zip(cache_state(a), cache_state(b)):
            assert np.array_equal(x, y), (parents, x, y)
        assert a.pages_free == b.pages_free
        refcount_is_the_number_of_table_entries(a)
        a._device_table()
        assert a.table_uploads == uploads + int(changed), parents
        if rows is not None:
            got = gathered(a)
            for s, p in enumerate(parents):
                assert np.array_equal(got[s], rows[p] if p >= 0 else rows[0][:0]), (parents, s)
        grow = [cache_rows(100 + step * 5 + s, 1 + (step + s) % 3) if a.lengths[s] else None for s in range(5)]
        if step % 2 == 0 and any(r is not None for r in grow):
            for cache in caches:                                                       # the sequences grow apart: copy-on-write
                cache_append(D, cache, grow)
            for x, y in zip(cache_state(a), cache_state(b)):
                assert np.array_equal(x, y), parents
            refcount_is_the_number_of_table_entries(a)
        if not a.lengths.any():
            for cache in caches:
                cache_append(D, cache, [cache_rows(200 + step + s, 20 + 7 * s) for s in range(4)] + [None])
        step += 1


def reorder_contiguous_equals_numpy(D, dtype='f32'):
    """A swap, a chain, all-to-one and an emptied slot on a contiguous cache: ``k[parents]``."""
    cache = D.KVCache(4, 48, 2, 16, dtype=dtype)
    lengths = [20, 7, 13, 0]
    cache_append(D, cache, [cache_rows(b, n) if n else None for b, n in enumerate(lengths)])
    for parents in ([1, 0, 2, 3], [1, 2, 0, -1], [0, 1, 2, 3], [2, 2, 2, 2], [3, 0, -1, 1], [1, 1, 0, 0]):
        rows = gathered(cache)
        before = len(rows)
        cache.reorder(parents)
        got = gathered(cache)
        assert cache.lengths.tolist() == [len(rows[p]) if p >= 0 else 0 for p in parents] and before == 4
        for s, p in enumerate(parents):
            assert np.array_equal(got[s], rows[p] if p >= 0 else rows[0][:0]), (parents, s)
        if not cache.lengths.any():
            break
        cache_append(D, cache, [cache_rows(50 + s, 2) if cache.lengths[s] else None for s in range(4)])


def reorder_bad_vectors(D, pytest):
    for cache in (D.PagedKVCache(3, 64, 2, 16, page_size=16), D.KVCache(3, 64, 2, 16)):
        cache_append(D, cache, [cache_rows(b, 20 + b) for b in range(3)])
        before = cache_state(cache)
        for parents, error in (([0, 1], ValueError), ([0, 1, 2, 0], ValueError), ([0.0, 1.0, 2.0], ValueError), ([True, False, True], ValueError),
                               ([[0, 1, 2]], ValueError), ([0, 1, 3], IndexError), ([0, -2, 1], IndexError)):
            with pytest.raises(error):
                cache.reorder(parents)
        assert all(np.array_equal(x, y) for x, y in zip(before, cache_state(cache)))


def reordered_sequences_equal_sequences_filled_on_their_own(npm, dtype, options, page_size):
    """One prompt in slot 0, three beams by ``reorder([0, 0, 0])``, then steps in which the beams are permuted, duplicated,
    dropped and revived by ``reorder`` while one token each is appended -- against a cache in which every slot holds the whole
    sequence its final occupant went through, fed in the same chunks.  The layer's outputs are compared as bits, step by step
    along every slot's line of ancestors.  ``page_size`` None: a contiguous cache, whose ``reorder`` copies rows."""
    import window_cases as WC
    f, heads, kv_heads = 64, 4, 2
    options = dict(options)
    window = options.pop('window', None)
    att, _ = WC.make_mha(npm, f, heads, kv_heads, seed=9, window=window, batch=3, **options)
    paging = {} if page_size is None else dict(page_size=page_size)
    rng = np.random.default_rng(page_size or 1)
    prompt = rng.standard_normal([37, f]).astype(np.float32)
    steps = [([0, 0, 0], [1, 1, 1]), ([1, 0, 2], [1, 1, 1]), ([2, 2, 0], [1, 1, 1]), ([0, 1, 2], [1, 1, 1]), ([1, 1, -1], [1, 1, 0]),
             ([0, 0, 1], [1, 1, 1]), ([2, 1, 0], [1, 1, 1])]
    tokens = rng.standard_normal([len(steps), 3, f]).astype(np.float32)
    cache = att.make_cache(3, 48, dtype=dtype, **paging)
    x = np.zeros([3, 37, f], dtype=np.float32)
    x[0] = prompt
    att(x, cache=cache, new_lengths=[37, 0, 0])
    line = [[], None, None]                                                            # per slot: the slot it sat in at every step so far
    got = []
    for s, (parents, n) in enumerate(steps):
        cache.reorder(parents)
        line = [None if p < 0 or line[p] is None else line[p] + [b] for b, p in enumerate(parents)]
        got.append(np.asarray(att(tokens[s][:, None], cache=cache, new_lengths=n)))
        if cache.paged:
            named = np.bincount(cache.block_table[cache.block_table >= 0], minlength=cache.pages)
            assert np.array_equal(cache.refcount, named)
        assert cache.lengths.tolist() == [0 if l is None else 37 + len(l) for l in line]
    assert all(l is not None and len(l) == len(steps) for l in line)
    if cache.paged and window is None and page_size == 16:
        assert cache.page_copies > 0 and cache.pages_in_use < 3 * -(-cache.max_length // page_size)
    own = att.make_cache(3, 48, dtype=dtype, **paging)
    att(np.repeat(prompt[None], 3, axis=0), cache=own)
    for s in range(len(steps)):
        fed = np.stack([tokens[s][line[b][s]] for b in range(3)])
        want = np.asarray(att(fed[:, None], cache=own))
        for b in range(3):
            assert np.array_equal(got[s][line[b][s]].view(np.uint32), want[b].view(np.uint32)), f'step {s}, the ancestor of slot {b}'


# ---- end to end: the tiny model of tests/test_gpu_generate.py ----------------------------------------------------------------------------
F, HEADS, HIDDEN, VOCAB = 32, 2, 64, 50
PROMPTS = (5, 1, 3)
DECODE_TOLERANCE = 1e-5                    # of max |logit|: what the decode tests allow between two ways of computing a logit


def tiny_model(npm):
    """(decoder, embedding, head, memory [3, 7, F], prompts [3, 5] padded with -1): tests/test_gpu_generate.py's fixture."""
    import decode_cases as DC
    dec, _ = DC.make_decoder(npm, F, HEADS, HEADS, HIDDEN, norm_first=True, causal=True, seed=40, batch=3, seq_kv=7)
    np.random.seed(41)
    emb = npm.layers.Embedding(VOCAB, F)
    emb(np.zeros([1], dtype=np.int64))
    head = npm.layers.Linear(units=VOCAB)
    head(np.zeros([1, F], dtype=np.float32))
    head._w.set(np.asarray(head._w) * np.float32(2.0 / np.sqrt(F)))
    rng = np.random.default_rng(42)
    kv = rng.standard_normal([3, 7, F]).astype(np.float32)
    prompt = np.full([3, max(PROMPTS)], -1, dtype=np.int64)
    for b, n in enumerate(PROMPTS):
        prompt[b, :n] = rng.integers(0, VOCAB, size=n)
    return dec, emb, head, kv, prompt


def greedy_tokens(npm, model, groups, steps):
    """[steps, groups]: the plain one-token loop with a greedy ``Sampler`` (tests/test_gpu_generate.py ``_generate``)."""
    from np_modeling_amd import device as D
    dec, emb, head, kv, prompt = model
    lengths = np.array(PROMPTS[:groups])
    width = int(lengths.max())
    state = dec.start_decoding(kv[:groups], 16, page_size=16, pages=groups)
    sampler = npm.sampling.Sampler(groups)
    x = emb.forward(prompt[:groups, :width])
    new_lengths, last = lengths, np.arange(groups) * width + lengths - 1
    tokens = []
    for _ in range(steps):
        hidden = dec.decode(x, state, new_lengths=new_lengths)
        result = sampler(head(D.take_rows(hidden.reshape(-1, F), last)))
        x = emb.forward(result.ids).reshape(groups, 1, F)
        tokens.append(result.numpy().tolist())
        new_lengths, last = None, np.arange(groups)
    return np.array(tokens)


def beam_flow(npm, model, groups, width, eos, max_new_tokens, **kwargs):
    """``beam.decode_step`` until every group is done, with ``beam_reference.PyBeamSearch`` run beside it on the logits copied to
    the host at each step; parents and tokens are asserted equal step by step (the next step's logits depend on them), and after
    every reorder the pages in use are the pages live beams name.  Returns (search, reference, the logits of every step)."""
    dec, emb, head, kv, prompt = model
    batch = groups * width
    state = dec.start_decoding(np.repeat(kv[:groups], width, axis=0), 16, page_size=16, pages=2 * batch)
    search = npm.beam.BeamSearch(groups, width, eos=eos, max_new_tokens=max_new_tokens, **kwargs)
    reference = BR.PyBeamSearch(groups, width, eos=eos, max_new_tokens=max_new_tokens, **kwargs)
    chunk, n = np.full([batch, max(PROMPTS)], -1, dtype=np.int64), np.zeros([batch], dtype=np.int64)
    chunk[::width], n[::width] = prompt[:groups], PROMPTS[:groups]
    seen = []

    def spy(x):
        logits = head(x)
        seen.append(logits.numpy())
        return logits

    first, done = (chunk, n), np.zeros([groups], dtype=bool)
    while not done.all():
        assert len(seen) <= max_new_tokens
        uploads = state.self_cache.table_uploads
        done = npm.beam.decode_step(dec, state, emb, spy, search, prompt=first)
        first = None
        parents, ids, ref_done = reference.search(seen[-1])
        assert search.step.parents.tolist() == parents.tolist() and search.step.host_ids.tolist() == ids.tolist(), len(seen)
        assert search.step.ids.numpy().tolist() == ids.tolist() and done.tolist() == ref_done.tolist()
        assert np.array_equal(search.scores().view(np.uint32), search.step.scores.view(np.uint32))
        cache = state.self_cache
        per_group = cache.lengths.reshape(groups, width)
        assert ((cache.lengths > 0) == (parents >= 0)).all() and ((per_group == per_group.max(axis=1, keepdims=True)) | (per_group == 0)).all()
        named = cache.block_table[parents >= 0]
        assert cache.pages_in_use == np.unique(named[named >= 0]).size
        assert cache.table_uploads <= uploads + 1
    return search, reference, seen


def least_decision_gap(reference, seen, vocab):
    """The least gap between two scores whose order decided something in the reference run, over 100 times the bound on what
    the device may differ by: eps at the largest |score| plus the decode tolerance at the largest |logit|.  At least 1 for a
    fixture the device must reproduce."""
    largest = max(float(np.abs(z[np.isfinite(z)]).max()) for z in seen)
    score = max([abs(s) for s in reference.scores_seen] + [1.0])
    bound = BR.eps(score, vocab) + DECODE_TOLERANCE * largest
    return min(reference.gaps) / (100 * bound)
