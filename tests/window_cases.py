"""Sliding-window attention over a key / value cache, restated: shared by tests/hostsim/ (profile 'window'), tests/test_window_host.py
(CPU) and tests/test_gpu_window.py (MI355X).

The rule (include/npm_hip.h npm_mha_decode_fwd_window).  Row t < n[b] of sequence b has the causal upper limit
limit = L[b] - n[b] + t + 1 and sees keys max(0, limit - W) <= j < limit.  Nothing below a row's floor enters its result.

* ``smallest_floor``: the floor of a sequence's first new token, max(0, L - n + 1 - W): no row at or past it is dead, and every row
  below it may hold anything (the GPU tests fill them with NaN).
* ``attention``: float64, one sequence at a time through tests/attn_range_data.reference with the band as a mask over rows
  smallest_floor .. L - 1 ONLY -- rows below are not even handed to the reference.
* ``band``: the [S, S] mask of a whole sequence, tril & ~tril(-W).
* ``poison`` / ``build_pool``: NaN below every sequence's smallest floor and at and past its length; the paged form also fills
  unused pages and makes every table entry of a reclaimed or out-of-range slot name an all-NaN page that is in range.
* ``held_slots``: which table slots a windowed ``PagedKVCache`` holds after a call, from first principles.
"""

import numpy as np

import attn_range_data as R


def smallest_floor(kv_lens, new_lens, window):
    kv_lens, new_lens = np.asarray(kv_lens, dtype=np.int64), np.asarray(new_lens, dtype=np.int64)
    return np.maximum(kv_lens - new_lens + 1 - int(window), 0)


def band(seq, window):
    tril = np.tril(np.ones([seq, seq], dtype=bool))
    return tril if window is None else tril & ~np.tril(np.ones([seq, seq], dtype=bool), -int(window))


def attention(q, k, v, kv_lens, new_lens, scale, window):
    """q [B, T, Hq, D], k / v [B, capacity, Hkv, D] -> ctx [B, T, Hq, D], lse [B, Hq, T] in float64; every sequence alone, rows
    without a visible key ctx = 0, lse = -inf."""
    b, tokens, hq, d = q.shape
    ctx = np.zeros([b, tokens, hq, d])
    lse = np.full([b, hq, tokens], -np.inf)
    first = smallest_floor(kv_lens, np.full(b, tokens) if new_lens is None else new_lens, window)
    for i in range(b):
        length, n = int(kv_lens[i]), int(tokens if new_lens is None else new_lens[i])
        if n == 0 or length == 0:
            continue
        assert n <= length
        keys = np.arange(int(first[i]), length)
        limit = length - n + np.arange(n) + 1
        mask = (keys[None, :] < limit[:, None]) & (keys[None, :] >= (limit - int(window))[:, None])
        out = R.reference(q[i:i + 1, :n], k[i:i + 1, keys[0]:length], v[i:i + 1, keys[0]:length], None, scale, mask=mask[None, None],
                          grads=False)
        ctx[i, :n], lse[i, :, :n] = out['ctx'][0], out['lse'][0]
    return ctx, lse


def poison(q, k, v, kv_lens, new_lens, window, fill=np.nan):
    """Cache rows below each sequence's smallest floor and at and past its length, and the padded query rows, hold ``fill``."""
    q, k, v = q.copy(), k.copy(), v.copy()
    rows = np.arange(k.shape[1])[None, :]
    n = np.full(len(kv_lens), q.shape[1]) if new_lens is None else np.asarray(new_lens)
    dead = (rows >= np.asarray(kv_lens)[:, None]) | (rows < smallest_floor(kv_lens, n, window)[:, None])
    k[dead], v[dead] = fill, fill
    q[np.arange(q.shape[1])[None, :] >= n[:, None]] = fill
    return q, k, v


def build_pool(k, v, kv_lens, new_lens, window, page_rows, order, seed=0, spare=3):
    """tests/paged_cases.build_pool for a windowed call: only the pages that hold a row in smallest_floor .. L - 1 exist.  Every
    other table entry -- below the first live page (reclaimed) or past the last -- names an unused all-NaN page that is in range;
    ``k`` / ``v`` are expected poisoned (``poison``), so the rows of a live page below the floor or past the length are NaN too.
    Returns pool_k, pool_v [pages, page_rows, ...], table int32 [B, P]."""
    b = len(kv_lens)
    per = max(-(-max(int(np.max(kv_lens)), 1) // page_rows), 1)
    pages = b * per + spare
    rng = np.random.default_rng(seed)
    ids = np.arange(b * per) if order == 'identity' else rng.permutation(pages)[:b * per]
    unused = np.setdiff1d(np.arange(pages), ids)
    first = smallest_floor(kv_lens, new_lens, window)
    table = np.empty([b, per], dtype=np.int32)
    pools = [np.full((pages, page_rows) + x.shape[2:], np.nan, dtype=np.float32) for x in (k, v)]
    for i in range(b):
        table[i] = unused[(i + np.arange(per)) % len(unused)]
        if kv_lens[i] == 0:
            continue
        for slot in range(int(first[i]) // page_rows, (int(kv_lens[i]) - 1) // page_rows + 1):
            table[i, slot] = ids[i * per + slot]
            take = min(page_rows, int(kv_lens[i]) - slot * page_rows)
            for pool, x in zip(pools, (k, v)):
                pool[table[i, slot], :take] = x[i, slot * page_rows:slot * page_rows + take]
    return pools[0], pools[1], table


def held_slots(length_before, length_after, window, page_rows, slots):
    """[slots] bool: the table slots a sequence holds after an append took it from ``length_before`` to ``length_after`` rows --
    the pages that hold a row >= length_before - window + 1 (what the append could not yet give back) or a row of the new range,
    below length_after."""
    rows = np.arange(slots * page_rows).reshape(slots, page_rows)
    return ((rows >= length_before - window + 1) & (rows < length_after)).any(axis=1)


def max_pages(window, tokens, page_rows):
    """Pages one sequence holds at most between calls of ``tokens`` tokens."""
    return -(-(window - 1 + tokens) // page_rows) + 1


# ---- layers -------------------------------------------------------------------------------------------------------------------
def make_mha(npm, features, heads, kv_heads, seed, window, batch=2, **kwargs):
    """tests/decode_cases.make_mha with ``window=`` (None: the keyword is not even passed)."""
    import decode_cases as DC
    np.random.seed(seed)
    if window is not None:
        kwargs['window'] = window
    att = npm.layers.MultiHeadAttention(heads, num_kv_heads=kv_heads, **kwargs)
    att(np.zeros([batch, 2, features], dtype=np.float32))
    for name in ('_wq', '_wk', '_wv', '_wo'):
        arr = getattr(att, name)
        arr.set(np.asarray(arr) * np.float32(2.0 / np.sqrt(features)))
    return att, {n: np.asarray(getattr(att, '_' + n)).astype(np.float64) for n in DC.ATT}


def make_decoder(npm, features, heads, kv_heads, hidden, norm_first, seed, window, batch=2, seq_kv=7, **kwargs):
    """tests/decode_cases.make_decoder, causal, with ``window=`` (None: the keyword is not even passed)."""
    import decode_cases as DC
    np.random.seed(seed)
    if window is not None:
        kwargs['window'] = window
    dec = npm.layers.TransformerDecoder(num_heads=heads, hidden_units=hidden, norm_first=norm_first, num_kv_heads=kv_heads,
                                        causal=True, **kwargs)
    dec(np.zeros([batch, 2, features], dtype=np.float32), np.zeros([batch, seq_kv, features], dtype=np.float32))
    for path, attrs in (('_self_attention', ('_wq', '_wk', '_wv', '_wo')), ('_cross_attention', ('_wq', '_wk', '_wv', '_wo')),
                        ('_dense1._linear', ('_w',)), ('_dense2', ('_w',))):
        for attr in attrs:
            arr = getattr(DC.sub(dec, path), attr)
            arr.set(np.asarray(arr) * np.float32(2.0 / np.sqrt(features)))
    return dec, DC.decoder_params(dec)
