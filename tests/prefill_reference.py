"""The prefill attention kernel, restated: shared by tests/test_prefill_host.py (CPU) and tests/test_gpu_prefill.py.

The rule is npm_mha_decode_fwd_varlen's (tests/varlen_reference.py) without the limit on the rows: sequence b brings n[b] <= T of
the T padded query rows and has L[b] valid cache rows with those included; row t < n[b] sees keys j <= L[b] - n[b] + t (causal) or
j < L[b]; a row without a visible key is ctx = 0, lse = -inf.  The float64 reference of every comparison stays
``varlen_reference.decode_attention``: every sequence alone.

* ``tokens_per_block``: R, the tokens one block of mha_prefill_kernel covers at a grouping (64 rows of (query head, token) pairs).
* ``kernel_cases``: the case grid of the GPU kernel test -- D x heads x T in {1, 33, R - 1, R, R + 1, 2 R + 3} x causal, each with a
  length set (tests/varlen_reference.LENGTH_SETS with max <= 700, plus one at the tile and page edges), a pitch layout and a way
  of placing the new tokens drawn round robin: 'top' puts n[b] new tokens ON TOP of the set's rows (L - n > 0: a chunk onto
  cached rows; the set's 0 gives L - n = 0 beside them), 'clip' keeps L and brings at most L tokens (a prefill from empty).
* ``group_cases``: a second grid, same tuples, at the groupings ``kernel_cases`` cannot reach: Hq / Hkv in {3, 5, 7} leaves the
  64-row tile partly filled (63, 60, 63 rows: ``tile_rows``), Hq / Hkv in {72, 65} needs a second head chunk that is partly full
  (``head_chunks``); T in {1, R, R + 1, 2 R + 3} (and 33 where R = 1), two head sizes per grouping.
* ``range_cases`` / ``range_data``: tests/attn_range_data.py's shifted (+-200) and saturated (nearly one-hot) scores at prefill
  shapes -- B 2, L 300 (19 key tiles); ``repeat_cases``: the three shapes the same call is repeated at.
* ``tile_model``: a float32 model of the kernel's accumulation order -- 16-key tiles in order, the raw running maximum, the
  online rescale of sum and accumulator per tile, one division at the end; the walk stops at the row's own limit.
* ``fractions``: the largest fraction of tests/decode_gpu.check's bound a result uses (the same formula, returned not asserted),
  so that the CPU test can hold the model to HALF of the GPU bound on exactly the GPU grid.
"""

import itertools

import numpy as np

import attn_range_data as R
import varlen_reference as VR

ROWS = 64                       # query rows per block of mha_prefill_kernel
TILE = 16                       # keys per tile
HEAD_DIMS = (16, 32, 64, 128)
HEADS = ((8, 8), (8, 2), (8, 1), (6, 3))
LENGTH_SETS = tuple(s for s in VR.LENGTH_SETS if max(s) <= 700) + ((15, 16, 17, 64, 65, 700),)
PAGE_SIZES = (16, 64)


def tokens_per_block(hq, hkv):
    return ROWS // min(hq // hkv, ROWS)


def token_counts(hq, hkv):
    r = tokens_per_block(hq, hkv)
    return sorted({1, 33, r - 1, r, r + 1, 2 * r + 3})


def _drawn(i, d, hq, hkv, t, causal):
    """Case ``i`` of a grid: its length set, pitch layout and placement drawn round robin."""
    base = np.array(LENGTH_SETS[(i * 3 + i // len(LENGTH_SETS)) % len(LENGTH_SETS)], dtype=np.int64)
    place = ('top', 'clip')[(i // 3) % 2]
    n = VR.new_lengths(t, np.full(len(base), t), 0, i)                    # the pattern T, 1, 0, T, T - 1, 1, shifted
    if place == 'top':
        lengths = base + n
    else:
        lengths = base
        if causal:
            n = np.minimum(n, lengths)
    return d, hq, hkv, t, causal, lengths, n, bool((i // 2) % 2), place


def kernel_cases():
    """(d, hq, hkv, t, causal, lengths, n, packed, place)."""
    out = []
    for d, (hq, hkv) in itertools.product(HEAD_DIMS, HEADS):
        for t, causal in itertools.product(token_counts(hq, hkv), (0, 1)):
            out.append(_drawn(len(out), d, hq, hkv, t, causal))
    return out


GROUP_HEADS = ((12, 4), (5, 1), (7, 1), (72, 1), (130, 2))      # groups 3, 5, 7 (a partly filled tile); 72, 65 (two head chunks)
EDGE_SET = LENGTH_SETS[-1]


def tile_rows(hq, hkv):
    """gb tb: the rows of a block's 64-row tile that are (query head, token) pairs at all."""
    gb = min(hq // hkv, ROWS)
    return gb * (ROWS // gb)


def head_chunks(hq, hkv):
    """(blocks per token tile a group is spread over, heads of the last one)."""
    group = hq // hkv
    gb = min(group, ROWS)
    chunks = -(-group // gb)
    return chunks, group - (chunks - 1) * gb


def group_token_counts(hq, hkv):
    r = tokens_per_block(hq, hkv)
    return sorted({1, r, r + 1, 2 * r + 3} | ({33} if hq // hkv >= ROWS else set()))


def group_cases():
    """``kernel_cases``' tuples at GROUP_HEADS; grouping g runs at head sizes HEAD_DIMS[g % 4] and HEAD_DIMS[(g + 2) % 4], so
    that every head size meets a partly filled tile and a second head chunk."""
    out = []
    for g, (hq, hkv) in enumerate(GROUP_HEADS):
        for d in (HEAD_DIMS[g % 4], HEAD_DIMS[(g + 2) % 4]):
            for t, causal in itertools.product(group_token_counts(hq, hkv), (0, 1)):
                out.append(_drawn(len(out), d, hq, hkv, t, causal))
    return out


def case_id(case):
    d, hq, hkv, t, causal, lengths, n, packed, place = case
    return f'D{d}-H{hq}/{hkv}-T{t}-c{causal}-L{"_".join(map(str, lengths))}-n{"_".join(map(str, n))}-{"packed" if packed else "plain"}-{place}'


def case_data(case):
    """q [B, T, Hq, D], k / v [B, capacity, Hkv, D] of a case, seeded by its shape."""
    d, hq, hkv, t, causal, lengths, n, packed, place = case
    rng = np.random.default_rng(d * 1000 + hq * 100 + t * 10 + causal + int(lengths.max()))
    b, cap = len(lengths), int(lengths.max()) + 3
    return (rng.standard_normal([b, t, hq, d]).astype(np.float32), rng.standard_normal([b, cap, hkv, d]).astype(np.float32),
            rng.standard_normal([b, cap, hkv, d]).astype(np.float32))


# ---- score range: tests/attn_range_data.py's constructions at prefill shapes -------------------------------------------------------
RANGE_SHAPES = ((128, 8, 2, 67), (64, 8, 8, 70), (32, 6, 3, 40), (16, 8, 1, 17), (64, 12, 4, 45))      # (D, Hq, Hkv, T)
RANGE_BATCH, RANGE_LEN = 2, 300                                           # 19 key tiles: both LDS buffers many times over
RANGE_KINDS = ('shift', 'saturated')


def range_cases():
    """(d, hq, hkv, t, kind, causal)."""
    return [s + (kind, causal) for s in RANGE_SHAPES for kind in RANGE_KINDS for causal in (0, 1)]


def range_id(case):
    d, hq, hkv, t, kind, causal = case
    return f'D{d}-H{hq}/{hkv}-T{t}-{kind}-c{causal}'


def range_data(d, hq, hkv, t, kind):
    """q [B, T, Hq, D], k, v [B, L, Hkv, D] and the scale.  'shift': every score of a row moved by up to +-200 (``shift_problem``'s
    k + u).  'saturated': nearly one-hot rows, and the largest scores of token 0 in the LAST key tile, at keys a causal row
    cannot see (tests/test_gpu_decode.py's construction)."""
    if kind == 'shift':
        q, _, v, _, scale, ku, _ = R.shift_problem(RANGE_BATCH, hq, hkv, t, RANGE_LEN, d, seed=d + t)
        return q, ku, v, scale
    q, k, v, _, scale = R.saturated_problem(RANGE_BATCH, hq, hkv, t, RANGE_LEN, d, seed=d + t + 1)
    k[:, -2] = 3.0 * np.sign(q[:, 0, :hkv])
    k[:, -1] = 6.0 * np.sign(q[:, 0, :hkv])
    return q, k, v, scale


def repeat_cases():
    """``kernel_cases``' tuples for the run-to-run test: T = 2 R + 3 at D 128 of the first grid, a partly filled tile, two head
    chunks; the sequences of each walk an odd and an even number of key tiles."""
    def case(d, hq, hkv, t, causal, lengths, n):
        return d, hq, hkv, t, causal, np.array(lengths, dtype=np.int64), np.array(n, dtype=np.int64), False, 'top'
    return [case(128, 8, 2, 35, 1, (304, 512, 17), (35, 35, 17)), case(64, 12, 4, 45, 0, (300, 45, 128), (45, 44, 1)),
            case(32, 72, 1, 5, 1, (65, 320, 5), (5, 4, 5))]


def tile_model(q, k, v, kv_lens, new_lens, scale, causal):
    """float32, the kernel's order: ctx [B, T, Hq, D], lse [B, Hq, T]."""
    f = np.float32
    b, tokens, hq, d = q.shape
    hkv = k.shape[2]
    c2 = f(f(scale) * f(R.LOG2E))
    ctx = np.zeros([b, tokens, hq, d], dtype=f)
    lse = np.full([b, hq, tokens], -np.inf, dtype=f)
    heads = np.arange(hq) % hkv
    for bi in range(b):
        length, n = int(kv_lens[bi]), int(tokens if new_lens is None else new_lens[bi])
        limit = np.where(np.arange(tokens) < n, (length - n + np.arange(tokens) + 1) if causal else length, 0)
        limit = np.clip(limit, 0, length)
        qb = q[bi].astype(f)                                                  # [T, Hq, D]
        m = np.full([tokens, hq], -np.inf, dtype=f)
        l = np.zeros([tokens, hq], dtype=f)
        acc = np.zeros([tokens, hq, d], dtype=f)
        for key0 in range(0, int(limit.max()), TILE):
            hi = min(key0 + TILE, length)
            kt, vt = k[bi, key0:hi][:, heads].astype(f), v[bi, key0:hi][:, heads].astype(f)      # [keys, Hq, D]
            s = np.einsum('thd,jhd->thj', qb, kt).astype(f)
            seen = (key0 + np.arange(hi - key0))[None, None, :] < limit[:, None, None]
            x = np.where(seen, s, f(-np.inf)).astype(f)
            m_new = np.maximum(m, x.max(axis=2))
            none = np.isneginf(m_new)
            ref = np.where(none, f(0), m_new * c2).astype(f)
            with np.errstate(invalid='ignore'):
                alpha = np.exp2(np.where(np.isneginf(m), f(-np.inf), m * c2 - ref)).astype(f)
                p = np.exp2((x * c2 - ref[:, :, None]).astype(f)).astype(f)
            m = m_new
            l = (l * alpha + p.sum(axis=2, dtype=f)).astype(f)
            acc = (acc * alpha[:, :, None] + np.einsum('thj,jhd->thd', p, vt).astype(f)).astype(f)
        some = ~np.isneginf(m)
        ctx[bi][some] = (acc[some] / l[some][:, None]).astype(f)
        lse[bi].T[some] = (f(scale) * m[some] + np.log2(l[some]).astype(f) * f(0.6931471805599453)).astype(f)
    return ctx, lse


def fractions(got_ctx, got_lse, q, k, v, kv_lens, new_lens, scale, causal):
    """(ctx, lse): the largest |got - float64| over tests/decode_gpu.check's bound, formula for formula; rows without a visible
    key must be exactly 0 / -inf."""
    t = q.shape[1]
    want_ctx, want_lse = VR.decode_attention(q, k, v, kv_lens, new_lens, scale, causal)
    seen = VR.valid_rows(t, kv_lens, new_lens)
    assert (got_ctx[~seen] == 0).all() and np.isneginf(got_lse.transpose(0, 2, 1)[~seen]).all()
    worst_ctx = worst_lse = 0.0
    for i in np.nonzero(seen.any(axis=1))[0]:
        rows = seen[i]
        g_ctx, g_lse = got_ctx[i, rows].astype(np.float64), got_lse[i][:, rows].astype(np.float64)
        assert np.isfinite(g_ctx).all() and np.isfinite(g_lse).all()
        x = R.exponent_magnitude(q[i:i + 1, rows], k[i:i + 1, :kv_lens[i]], scale, want_lse[i:i + 1, :, rows])
        worst_ctx = max(worst_ctx, float((np.abs(g_ctx - want_ctx[i, rows]) / (R.exponent_tol(2e-6, x) * (1.0 + np.abs(want_ctx[i, rows])))).max()))
        worst_lse = max(worst_lse, float(np.abs(g_lse - want_lse[i][:, rows]).max() / R.exponent_tol(3e-6, x)))
    return worst_ctx, worst_lse
