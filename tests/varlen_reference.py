"""Ragged batches in the key / value cache, restated: shared by tests/test_varlen_host.py (CPU) and tests/test_gpu_varlen.py.

The rule (include/npm_hip.h npm_mha_decode_fwd_varlen).  A call carries T padded query rows per sequence; sequence b brings
n[b] <= T of them and has L[b] valid cache rows with those included.  Row t < n[b] sees keys j <= L[b] - n[b] + t (causal) or
j < L[b]; a row without a visible key (t >= n[b], or L[b] = 0) is ctx = 0, lse = -inf.

* ``decode_attention``: float64, one sequence at a time through tests/decode_reference.decode_attention on that sequence's own
  unpadded rows -- the reference of every comparison is "sequence b run alone at batch 1".
* ``split_model``: tests/decode_reference.split_model's float32 model of the split / combine rule with the key ranges of the
  splits taken from ``lmax`` (the host's upper bound) and clipped to each sequence's own length: a split that starts at or past
  L[b] is empty (m = -inf, l = 0) and gets weight 0.
* ``kernel_cases``: the case grid of the GPU kernel test, so that the CPU test can hold the model to HALF of the GPU bound on
  exactly those (lengths, D, splits).
* ``layer_alone`` / ``decoder_alone``: float64 layer and decoder outputs of a ragged schedule, sequence by sequence.
"""

import itertools

import numpy as np

import attn_range_data as R
import decode_reference as DR

HEAD_DIMS = (16, 32, 64, 128)
HEADS = ((8, 8), (8, 4), (8, 2), (8, 1), (6, 3), (1, 1))        # tests/test_gpu_decode.py's
TOKENS = (1, 2, 5, 16)
MAX_ROWS = 32
# valid rows per sequence (the batch is their count): a tile edge (15, 16, 17), a split edge (the automatic rule cuts every 256
# keys: 255 .. 257, 512), one long sequence (>= 2049) beside short ones, and 0 (kept for the non-causal cases only)
LENGTH_SETS = ((1, 15, 16, 17), (0, 1, 17, 300), (2049, 5, 1, 256), (255, 256, 257, 16, 512), (4099, 33, 0, 1, 128, 2),
               (16, 16, 16), (3000, 2999, 1, 0, 47, 48, 49, 700))
SPLIT_MODES = ('one', 'auto', 'many', 2, 'auto', 32)


def new_lengths(tokens, lengths, causal, shift):
    """n[b] mixing 0, 1 and T (and T - 1), bounded by the sequence's own rows when the new tokens are among them."""
    pattern = (tokens, 1, 0, tokens, max(tokens - 1, 0), 1)
    n = np.array([pattern[(i + shift) % len(pattern)] for i in range(len(lengths))], dtype=np.int64)
    return np.minimum(n, lengths) if causal else n


def split_count(mode, lmax, batch, kv_heads):
    tiles = (lmax + DR.TILE - 1) // DR.TILE
    if mode == 'auto':
        return DR.auto_splits(batch, kv_heads, lmax) if lmax >= 1 else 1
    return {'one': 1, 'many': min(tiles + 3, 1024)}.get(mode, mode)


def kernel_cases():
    """(d, hq, hkv, t, causal, lengths, n, packed, mode): every (D, heads, T, causal) the kernel takes, each with a length set, a
    pitch layout and a split mode drawn round robin."""
    out, i = [], 0
    for d, (hq, hkv), t, causal in itertools.product(HEAD_DIMS, HEADS, TOKENS, (0, 1)):
        if hq // hkv * t > MAX_ROWS:
            continue
        lengths = np.array(LENGTH_SETS[(i * 3 + i // len(LENGTH_SETS)) % len(LENGTH_SETS)], dtype=np.int64)
        if causal:
            lengths = np.maximum(lengths, 1)
        n = new_lengths(t, lengths, causal, i)
        out.append((d, hq, hkv, t, causal, lengths, n, bool((i // 2) % 2), SPLIT_MODES[(i * 5 + i // 6) % 6]))
        i += 1
    return out


def case_id(case):
    d, hq, hkv, t, causal, lengths, n, packed, mode = case
    return f'D{d}-H{hq}/{hkv}-T{t}-c{causal}-L{"_".join(map(str, lengths))}-n{"_".join(map(str, n))}-{"packed" if packed else "plain"}-{mode}'


def decode_attention(q, k, v, kv_lens, new_lens, scale, causal):
    """q [B, T, Hq, D], k / v [B, capacity, Hkv, D] -> ctx [B, T, Hq, D], lse [B, Hq, T] in float64; every sequence alone."""
    b, tokens, hq, d = q.shape
    ctx = np.zeros([b, tokens, hq, d])
    lse = np.full([b, hq, tokens], -np.inf)
    for i in range(b):
        length, n = int(kv_lens[i]), int(tokens if new_lens is None else new_lens[i])
        if n == 0 or length == 0:
            continue
        assert not causal or n <= length
        ctx[i, :n], lse[i, :, :n] = (x[0] for x in DR.decode_attention(q[i:i + 1, :n], k[i:i + 1, :length], v[i:i + 1, :length],
                                                                          length, scale, causal))
    return ctx, lse


def valid_rows(tokens, kv_lens, new_lens):
    """[B, T] bool: the rows that have a visible key."""
    n = np.full(len(kv_lens), tokens) if new_lens is None else np.asarray(new_lens)
    return (np.arange(tokens)[None, :] < n[:, None]) & (np.asarray(kv_lens)[:, None] > 0)


def split_model(q, k, v, kv_lens, new_lens, scale, causal, splits, lmax):
    """The split / combine rule in float32 with the partition of ``lmax`` and per-sequence early exit.  ctx, lse as float32;
    a row without a visible key is 0 / -inf by selection."""
    f = np.float32
    b, tokens, hq, d = q.shape
    hkv = k.shape[2]
    c2 = f(f(scale) * f(R.LOG2E))
    ctx = np.zeros([b, tokens, hq, d], dtype=f)
    lse = np.full([b, hq, tokens], -np.inf, dtype=f)
    ranges = DR.split_ranges(lmax, splits)
    for bi in range(b):
        length, n = int(kv_lens[bi]), int(tokens if new_lens is None else new_lens[bi])
        limit = np.where(np.arange(tokens) < n, (length - n + np.arange(tokens) + 1) if causal else length, 0)
        visible = np.arange(length)[None, :] < limit[:, None]
        for h in range(hq):
            kp, vp = k[bi, :length, h % hkv].astype(f), v[bi, :length, h % hkv].astype(f)
            x = np.where(visible, (q[bi, :, h].astype(f) @ kp.T) * c2, f(-np.inf)).astype(f)
            parts = []
            for lo, hi in ranges:
                lo, hi = min(lo, length), min(hi, length)
                if hi <= lo:                                              # the block returns before it loads anything
                    parts.append((np.full(tokens, -np.inf, dtype=f), np.zeros(tokens, dtype=f), None))
                    continue
                xs = x[:, lo:hi]
                m = xs.max(axis=1)
                ref = np.where(np.isneginf(m), f(0), m).astype(f)
                p = np.exp2(xs - ref[:, None]).astype(f)
                parts.append((m.astype(f), p.sum(axis=1, dtype=f), (p @ vp[lo:hi]).astype(f)))
            top = np.max([m for m, _, _ in parts], axis=0)
            tot, acc = np.zeros(tokens, dtype=f), np.zeros([tokens, d], dtype=f)
            for m, l, a in parts:
                if a is None:
                    continue
                w = np.where(np.isneginf(m), f(0), np.exp2(np.where(np.isneginf(m), f(0), m - np.where(np.isneginf(top), f(0), top)))).astype(f)
                tot = (tot + l * w).astype(f)
                acc = (acc + a * w[:, None]).astype(f)
            some = ~np.isneginf(top)
            ctx[bi, some, h] = acc[some] / tot[some, None]
            lse[bi, h, some] = (top[some] + np.log2(tot[some])).astype(f) * f(0.6931471805599453)
    return ctx, lse


# ---- layers: a ragged schedule, every sequence alone ---------------------------------------------------------------------
def schedule_rows(schedule):
    """``schedule``: a list of n arrays [B] (tokens each sequence brings per call) -> tokens per sequence in total."""
    return np.sum(schedule, axis=0)


def padded_calls(x_rows, schedule, pad=0.0):
    """``x_rows``: list of B arrays [S_b, F] (each sequence's own tokens).  Returns per call (x [B, T, F] padded on the right with
    ``pad``, n [B]) with T = max n."""
    b, f = len(x_rows), x_rows[0].shape[1]
    at = np.zeros(b, dtype=np.int64)
    calls = []
    for n in schedule:
        n = np.asarray(n, dtype=np.int64)
        t = int(n.max())
        x = np.full([b, t, f], pad, dtype=x_rows[0].dtype)
        for i in range(b):
            x[i, :n[i]] = x_rows[i][at[i]:at[i] + n[i]]
        at += n
        calls.append((x, n))
    return calls


def layer_alone(p, x_rows, schedule):
    """Float64 cached self-attention of every sequence alone, fed in the chunks the schedule gives it: list of [S_b, F]."""
    out = []
    for i, rows in enumerate(x_rows):
        chunks = DR_split(rows[None].astype(np.float64), [int(n[i]) for n in schedule])
        out.append(DR.mha_cached(p, chunks)[0] if chunks else np.zeros([0, rows.shape[1]]))
    return out


def cross_alone(p, x_rows, kv, kv_lengths):
    """Float64 cross-attention of every sequence's rows over its own ``kv_lengths[b]`` memory rows."""
    out = []
    for i, rows in enumerate(x_rows):
        mem = np.asarray(kv[i:i + 1, :kv_lengths[i]], dtype=np.float64)
        cache = dict(k=DR._project(mem, p['wk'], p['bk']), v=DR._project(mem, p['wv'], p['bv']))
        out.append(DR.mha_cross_cached(p, rows[None].astype(np.float64), cache)[0])
    return out


def decoder_alone(p, q_rows, schedule, kv, kv_lengths, norm_first):
    """``decoder_cached`` of every sequence alone with its own chunks and its own memory rows: list of [S_b, F]."""
    out = []
    for i, rows in enumerate(q_rows):
        chunks = DR_split(rows[None].astype(np.float64), [int(n[i]) for n in schedule])
        mem = np.asarray(kv[i:i + 1, :kv_lengths[i]], dtype=np.float64)
        out.append(DR.decoder_cached(p, chunks, mem, norm_first)[0])
    return out


def DR_split(x, sizes):
    """``x`` [1, S, F] in chunks of ``sizes``, the empty ones (a sequence that rides along) left out."""
    edges = np.cumsum([0] + list(sizes))
    return [x[:, a:b] for a, b in zip(edges[:-1], edges[1:]) if b > a]


def collect(outs, schedule, batch):
    """The valid rows of the per-call outputs [B, T, F], concatenated per sequence: list of [S_b, F]."""
    rows = [[] for _ in range(batch)]
    for out, n in zip(outs, schedule):
        for i in range(batch):
            rows[i].append(np.asarray(out)[i, :n[i]])
    return [np.concatenate(r, axis=0) for r in rows]
