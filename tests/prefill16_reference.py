"""The case list of tests/test_gpu_prefill16.py: npm_mha_prefill_fwd_f16 against npm_mha_prefill_fwd on the rounded values, bitwise.

A case is (D, Hq, Hkv, T, L, causal, B, layout).  The axes are the ways the fp16 instance of the kernel can go wrong, at the
smallest shapes that reach them:
* D in {16, 32, 64, 128}: TILE D / 8 pieces of 8 halves a tile -- 32, 64 and 128 pieces for 256 threads (the partly used pass) and
  exactly one per thread at D 128 -- and the head offset c D in halves;
* (Hq, Hkv) in HEADS: 64, 16 and 32 tokens per block, and (72, 1): one token per block and two head chunks;
* T in {1, R, R + 1, 2 R + 3} for R tokens per block: one row, a full tile, a second tile with one row, three token tiles;
* L in LENGTHS: the tile edge (15, 16, 17: the redirect to key L - 1 and the zeroed V of a partly filled last tile), the edge of
  a 64-row page (64, 65) and 337 rows (22 tiles over 22 / 6 pages);
* the layouts of tests/kv16_reference.py, causal or not, batch 1 or 3.
The product of the first four axes has 360 members; every fifth and every fifth-plus-two of them is kept (144), and layout, causal
and batch are drawn round robin, so that every value of every axis meets every D (``test_prefill16_host.py`` asserts it).  The
uniform layout has no length arrays, so there L < T becomes T."""

import numpy as np

import decode_reference as DR
import kv16_reference as K16
import prefill_reference as PR
import varlen_reference as VR
from oracle import np_oracle as O

HEAD_DIMS = (16, 32, 64, 128)
HEADS = ((8, 8), (8, 2), (6, 3), (72, 1))
LENGTHS = (15, 16, 17, 64, 65, 337)
LAYOUTS = K16.LAYOUTS
BATCHES = (1, 3)


def token_counts(hq, hkv):
    r = PR.tokens_per_block(hq, hkv)
    return sorted({1, r, r + 1, 2 * r + 3})


def bitwise_cases():
    """(D, Hq, Hkv, T, L, causal, B, layout)."""
    full = [(d, hq, hkv, t, length) for d in HEAD_DIMS for hq, hkv in HEADS for t in token_counts(hq, hkv) for length in LENGTHS]
    out = []
    for i, (d, hq, hkv, t, length) in enumerate(full):
        if i % 5 not in (0, 2):
            continue
        k = len(out)
        layout = LAYOUTS[(k + k // 8) % 4]
        out.append((d, hq, hkv, t, max(length, t) if layout == 'uniform' else length, (k // 4 + k // 16) % 2, BATCHES[(k // 2 + k // 8) % 2],
                    layout))
    return out


def case_id(c):
    return 'D%d-H%d/%d-T%d-L%d-c%d-B%d-%s' % c


def lengths(b, t, length, layout, causal):
    """(kv_lens, new_lens) of a case, as tests/test_gpu_kv16.py's ``_lengths``: the uniform call has none; the others include a
    sequence without rows and a padded token.  Causal: the new tokens are among the valid rows."""
    if layout == 'uniform':
        return None, None
    if b == 1:
        kv, new = [length], [max(t - 1, 1)]
    else:
        third = max(length - 3, 1)
        kv, new = [length, 0, third], [t, 0, max(t - 1, 1)]
    kv, new = np.array(kv, dtype=np.int32), np.array(new, dtype=np.int32)
    return kv, np.minimum(new, kv) if causal else np.where(kv > 0, new, 0).astype(np.int32)



# ---- the float64 decoder over caches that store halves ------------------------------------------------------------------------
def _stored(x):
    """What an fp16 cache keeps of the float64 rows ``x``: the append rounds the float32 projection to fp16 (nearest even), and
    every later read converts it back exactly."""
    return K16.rounded(np.asarray(x, dtype=np.float32)).astype(np.float64)


def decoder_cached_stored(p, chunks, kv, norm_first, eps=1e-3, store=_stored):
    """tests/decode_reference.py's ``decoder_cached`` with K and V rounded to fp16 AT THE POINT OF STORAGE -- the rows of every
    chunk as they are appended to the self cache, the memory's projection as it fills the cross cache -- and everything else in
    float64: Q, scores, softmax, context, projections, norms and the feed-forward.  ``store`` replaces the rounding; with the
    identity the result is ``decoder_cached``'s exactly, which tests/test_gpu_prefill16.py asserts so that the two cannot drift."""
    sa, ca = O._att(p, 'sa'), O._att(p, 'ca')
    kv = np.asarray(kv, dtype=np.float64)
    cross = dict(k=store(DR._project(kv, ca['wk'], ca['bk'])), v=store(DR._project(kv, ca['wv'], ca['bv'])))
    rows = dict(k=None, v=None)
    scale = 1.0 / np.sqrt(sa['wq'].shape[1])
    norm = lambda x, n: O.layernorm_fwd(x, p[f'{n}_gamma'], p[f'{n}_beta'], eps)[0]
    outs = []
    for q in chunks:
        q = np.asarray(q, dtype=np.float64)
        b, t, f = q.shape
        h = norm(q, 'n1') if norm_first else q
        for name, w, bias in (('k', 'wk', 'bk'), ('v', 'wv', 'bv')):
            new = store(DR._project(h, sa[w], sa[bias]))
            rows[name] = new if rows[name] is None else np.concatenate([rows[name], new], axis=1)
        ctx, _ = DR.decode_attention(DR._project(h, sa['wq'], sa['bq']), rows['k'], rows['v'], rows['k'].shape[1], scale, True)
        out = np.einsum('...abc,...dbc->...ad', ctx, sa['wo']) + sa['bo'] + q
        if not norm_first:
            out = norm(out, 'n1')
        skip = out
        h = norm(out, 'n2') if norm_first else out
        out = DR.mha_cross_cached(ca, h, cross) + skip
        if not norm_first:
            out = norm(out, 'n2')
        out = out.reshape(-1, f)
        skip = out
        h = norm(out, 'n3') if norm_first else out
        h, _ = O.dense_fwd(h, p['d1_w'], p['d1_b'])
        out = O.linear_fwd(h, p['d2_w'], p['d2_b']) + skip
        if not norm_first:
            out = norm(out, 'n3')
        outs.append(out.reshape(b, t, f))
    return np.concatenate(outs, axis=1)


def decoder_alone_stored(p, q_rows, schedule, kv, kv_lengths, norm_first, store=_stored):
    """tests/varlen_reference.py's ``decoder_alone`` over fp16 caches: ``decoder_cached_stored`` of every sequence alone with its own
    chunks and its own memory rows: list of [S_b, F]."""
    out = []
    for i, rows in enumerate(q_rows):
        chunks = VR.DR_split(rows[None].astype(np.float64), [int(n[i]) for n in schedule])
        out.append(decoder_cached_stored(p, chunks, np.asarray(kv[i:i + 1, :kv_lengths[i]], dtype=np.float64), norm_first, store=store)[0])
    return out
