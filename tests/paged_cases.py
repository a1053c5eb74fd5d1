"""Shared by tests/test_paged_host.py (host simulator) and tests/test_gpu_paged.py (MI355X): page pools built from contiguous
caches, and the continuous-batching plan (four sequences decode, one is released, a fifth is admitted into its slot)."""

import numpy as np

import varlen_reference as VR

PAGE_SIZES = (16, 64)


def pages_of(length, page_rows):
    return -(-int(length) // page_rows)


def build_pool(k, v, lengths, page_rows, order, seed=0, spare=3):
    """Scatter the valid rows of contiguous caches ``k`` / ``v`` [B, capacity, ...] (any trailing shape) into page pools.

    ``order`` 'identity': sequence b owns pages b * P .. b * P + P - 1 (P = pages per sequence of the longest); 'random': a seeded
    permutation of more pages than needed.  NaN fills every row of a page past its sequence's length and every unused page;
    table entries past a sequence's last page name an unused (all-NaN) page, so every entry is in range and a kernel that forms
    an address from one reads NaN, never out of bounds.  Returns pool_k, pool_v [pages, page_rows, ...], table int32 [B, P]."""
    b = len(lengths)
    per = max(pages_of(max(int(np.max(lengths)), 1), page_rows), 1)
    pages = b * per + spare
    rng = np.random.default_rng(seed)
    ids = np.arange(b * per) if order == 'identity' else rng.permutation(pages)[:b * per]
    unused = np.setdiff1d(np.arange(pages), ids)
    assert len(unused) >= spare
    table = np.empty([b, per], dtype=np.int32)
    pools = [np.full((pages, page_rows) + x.shape[2:], np.nan, dtype=np.float32) for x in (k, v)]
    for i in range(b):
        own = pages_of(lengths[i], page_rows)
        table[i, :own] = ids[i * per:i * per + own]
        table[i, own:] = unused[(i + np.arange(per - own)) % len(unused)]
        for first in range(0, int(lengths[i]), page_rows):
            take = min(page_rows, int(lengths[i]) - first)
            for pool, x in zip(pools, (k, v)):
                pool[table[i, first // page_rows], :take] = x[i, first:first + take]
    return pools[0], pools[1], table


def extra_kernel_cases():
    """Cases in the form of tests/varlen_reference.kernel_cases() with lengths AT a multiple of the page sizes 16 and 64 and one
    past it, which not every length set of that grid has."""
    out = []
    sets = ((64, 65, 128, 129, 16, 17), (1024, 1025, 63, 64, 1, 4096), (4097, 192, 193, 32, 33))
    i = 0
    for d in VR.HEAD_DIMS:
        for (hq, hkv), t in (((8, 2), 1), ((8, 8), 4), ((6, 3), 5), ((8, 1), 2)):
            for causal in (0, 1):
                lengths = np.array(sets[i % len(sets)], dtype=np.int64)
                n = VR.new_lengths(t, lengths, causal, i)
                out.append((d, hq, hkv, t, causal, lengths, n, bool(i % 2), VR.SPLIT_MODES[i % 6]))
                i += 1
    return out


# ---- continuous batching -----------------------------------------------------------------------------------------------------
# Five logical sequences over four slots.  Sequence 1 ends after step RELEASE_AFTER and sequence 4 takes its slot at step ADMIT_AT.
SLOT = (0, 1, 2, 3, 1)
RELEASE_AFTER, ADMIT_AT = 3, 5
PLAN = [np.array(n) for n in ([5, 19, 3, 9, 0], [1, 1, 1, 1, 0], [1, 1, 1, 1, 0], [2, 1, 1, 0, 0],
                              [1, 0, 1, 1, 0],                       # slot 1 is empty and rides along
                              [1, 0, 1, 1, 7],                       # the fifth sequence's prompt beside single tokens
                              [1, 0, 1, 1, 1], [1, 0, 0, 1, 1], [1, 0, 1, 1, 1])]


def plan_rows():
    return VR.schedule_rows(PLAN)


def physical_calls(x_rows, pad=0.0):
    """Per step (x [4, T, F], n [4], logical n [5]): the padded chunk of the four slots."""
    calls = []
    for step, (x5, n5) in enumerate(VR.padded_calls(x_rows, PLAN, pad)):
        x = np.full([4, x5.shape[1], x5.shape[2]], pad, dtype=x5.dtype)
        n = np.zeros(4, dtype=np.int64)
        for seq in range(5):
            if n5[seq]:
                assert n[SLOT[seq]] == 0
                x[SLOT[seq]], n[SLOT[seq]] = x5[seq], n5[seq]
        calls.append((x, n, n5))
    return calls


def collect(outs):
    """Per-step outputs [4, T, F] -> the valid rows of each of the five sequences, concatenated."""
    logical = []
    for out, n5 in zip(outs, PLAN):
        out = np.asarray(out)
        wide = np.zeros((5,) + out.shape[1:], dtype=out.dtype)
        for seq in range(5):
            if n5[seq]:
                wide[seq] = out[SLOT[seq]]
        logical.append(wide)
    return VR.collect(logical, PLAN, 5)


def poison_pages(cache, pages):
    """NaN into whole pages of both pools (what a released sequence leaves behind must reach nothing)."""
    for arr in (cache.k, cache.v):
        host = np.asarray(arr).copy()
        host[np.asarray(pages, dtype=np.int64)] = np.nan
        arr.set(host)


def run_continuous(step, release, admit, cache, x_rows, pad=0.0):
    """The plan through ``step(x, n) -> out [4, T, F]``; ``release(slot)`` after step RELEASE_AFTER (its pages are then filled
    with NaN) and ``admit(slot)`` before step ADMIT_AT.  ``cache``: the paged self-attention cache.  Returns the five sequences'
    rows."""
    outs = []
    for i, (x, n, _) in enumerate(physical_calls(x_rows, pad)):
        if i == ADMIT_AT:
            admit(SLOT[4])
        out = np.asarray(step(x, n))
        assert np.isfinite(out).all(), f'step {i}: not finite'
        outs.append(out)
        if i == RELEASE_AFTER:
            pages = cache.block_table[SLOT[1]]
            pages = pages[pages >= 0].copy()
            assert len(pages) == pages_of(plan_rows()[1], cache.page_size)
            before = cache.pages_free
            release(SLOT[1])
            assert cache.pages_free == before + len(pages) and cache.lengths[SLOT[1]] == 0
            poison_pages(cache, pages)
    return collect(outs)
