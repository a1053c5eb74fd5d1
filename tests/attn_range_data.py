"""Data builders, a float64 reference and a model of the lazy online-softmax rule for tests/test_gpu_attn_range.py.

CPU only: nothing here touches the GPU (tests/test_attn_range_host.py checks the constructions without one).

The fused forward kernels (np_modeling_amd/csrc/npm_attn.hip, mha_fwd_kernel and mha_fwd8_kernel) keep, per query row, a
reference point m (log2 units of the scaled score) instead of the running maximum.  Per 32-key tile: tmax = the row's
largest scaled score * log2(e); if ANY row of the wave has tmax > m + 10, every row of the wave moves to
m_new = max(m, tmax) and multiplies its running sum l and its accumulators by alpha = 2^(m - m_new).  A wave holds 32
consecutive queries in mha_fwd_kernel and 16 in mha_fwd8_kernel.  ``simulate_lazy`` restates that rule, so that the
constructions below can be shown to reach it: moves after the first tile, alpha strictly inside (0, 1) on rows that did
not trigger, probabilities near 2^10 against the reference point.
"""

import numpy as np

LOG2E = 1.4426950408889634
EPS32 = 2.0 ** -24                     # unit roundoff of float32
RESCALE = 10.0                         # the kernels' threshold, log2 units
TILE = 32                              # keys per forward tile
WAVES = (16, 32)                       # queries per wave: mha_fwd8_kernel, mha_fwd_kernel


# ---- float64 reference -------------------------------------------------------------------------------------------
def reference(q, k, v, dctx, scale, mask=None, grads=True):
    """softmax(scale q k^T [masked]) v and its gradients in float64, one (b, h) plane at a time with np.matmul.
    q / dctx [B, Sq, Hq, D], k / v [B, Skv, Hkv, D]; query head h reads K / V head h % Hkv, dk / dv are the group sums.
    ``mask`` broadcasts to [B, Hq, Sq, Skv].  The same formulas as oracle/np_oracle.py attention_core_fwd / _bwd
    (tests/test_attn_range_host.py checks that), without their [B, H, Sq, Skv] einsum temporaries."""
    b, sq, h, d = q.shape
    skv, hkv = k.shape[1], k.shape[2]
    out = dict(ctx=np.zeros([b, sq, h, d]), lse=np.zeros([b, h, sq]))
    if grads:
        out.update(dq=np.zeros([b, sq, h, d]), dk=np.zeros([b, skv, hkv, d]), dv=np.zeros([b, skv, hkv, d]))
    full = None if mask is None else np.broadcast_to(mask, (b, h, sq, skv))
    for bi in range(b):
        for hi in range(h):
            c = hi % hkv
            qp, kp, vp = (np.asarray(x[bi, :, i], dtype=np.float64) for x, i in ((q, hi), (k, c), (v, c)))
            s = scale * (qp @ kp.T)
            if full is not None:
                s = np.where(full[bi, hi], s, -np.inf)
            top = s.max(axis=1, keepdims=True)
            e = np.exp(s - top)
            tot = e.sum(axis=1, keepdims=True)
            p = e / tot
            out['ctx'][bi, :, hi] = p @ vp
            out['lse'][bi, hi] = (top + np.log(tot))[:, 0]
            if grads:
                do = np.asarray(dctx[bi, :, hi], dtype=np.float64)
                dp = do @ vp.T
                ds = p * (dp - (p * dp).sum(axis=1, keepdims=True)) * scale
                out['dq'][bi, :, hi] = ds @ kp
                out['dk'][bi, :, c] += ds.T @ qp
                out['dv'][bi, :, c] += p.T @ do
    return out


def exponent_magnitude(q, k, scale, lse):
    """X = max |scale q.k| log2(e) + max |lse| log2(e), where |q.k| is taken as sum_d |q_d k_d| (the magnitude of the
    terms the score is summed from): the size, in log2 units, of the operands of the kernels' exponents."""
    h, hkv = q.shape[2], k.shape[2]
    top = 0.0
    for c in range(hkv):
        kk = np.abs(k[:, :, c].astype(np.float64))                      # [B, Skv, D]
        for hi in range(c, h, hkv):
            qq = np.abs(q[:, :, hi].astype(np.float64))                 # [B, Sq, D]
            top = max(top, float(np.matmul(qq, kk.transpose(0, 2, 1)).max()))
    return scale * top * LOG2E + float(np.abs(lse).max()) * LOG2E


X0 = 32.0                              # X of the O(1) data the existing bounds were set on (N(0,1) q, k at scale 1/sqrt(D))


def exponent_tol(base, x):
    """base * max(1, X / X0): the bound of tests/test_gpu_attn_range.py (derivation in its docstring)."""
    return base * max(1.0, x / X0)


# ---- the lazy reference point ------------------------------------------------------------------------------------
def simulate_lazy(s2, wave):
    """The kernels' rule on scaled scores in log2 units ``s2`` [Sq, Skv] (masked positions -inf).  Returns a dict:
    ``moves`` [Sq] number of tiles after the row's first visible one at which its reference point moved,
    ``alpha`` list of (row, tile, alpha) for rows that moved WITHOUT exceeding the threshold themselves,
    ``peak`` [Sq] largest 2^(s - m) met by the row (what l accumulates), ``first`` [Sq] first tile with a visible key."""
    sq, skv = s2.shape
    nt = (skv + TILE - 1) // TILE
    m = np.full(sq, -np.inf)
    moves = np.zeros(sq, dtype=int)
    peak = np.zeros(sq)
    first = np.full(sq, -1)
    alphas = []
    for t in range(nt):
        tmax = s2[:, TILE * t:TILE * t + TILE].max(axis=1)
        first[(first < 0) & np.isfinite(tmax)] = t
        for w0 in range(0, sq, wave):
            rows = slice(w0, min(w0 + wave, sq))
            over = tmax[rows] > m[rows] + RESCALE
            if not over.any():
                continue
            m_old = m[rows].copy()
            m_new = np.maximum(m_old, tmax[rows])
            moved = np.isfinite(m_old) & (m_new > m_old)
            moves[rows] += moved
            for r in np.nonzero(moved & ~over)[0]:
                alphas.append((w0 + r, t, 2.0 ** (m_old[r] - m_new[r])))
            m[rows] = m_new
        with np.errstate(invalid='ignore'):
            rel = np.where(np.isfinite(m)[:, None], s2[:, TILE * t:TILE * t + TILE] - m[:, None], -np.inf)
        peak = np.maximum(peak, np.exp2(rel).max(axis=1))
    return dict(moves=moves, alpha=alphas, peak=peak, first=first)


LAZY_SCALE = 2.0 ** -6                 # power of two: every scaled score is an exact multiple of 1/64
LAZY_KINDS = ('climb', 'under', 'edges', 'masked')
_NAT = 64                              # raw score units per natural unit at LAZY_SCALE
CLIMB, UNDER, GENTLE1, GENTLE2, DESCEND = 8 * _NAT, 421, 2 * _NAT, 5 * _NAT, -6 * _NAT   # raw rise per tile
# in log2 units per tile: 11.54 (> 10: a move on every tile), 9.49 (a move every other tile), 2.89, 7.21, -8.66


def _slopes(kind, i, b):
    """Per-row raw rise per tile, last-tile bump, first-tile bump (raw units) of construction ``kind``."""
    n = len(i)
    slope, last, first = np.zeros(n), np.zeros(n), np.zeros(n)
    j = (i + 3 * b) % 5 if kind == 'climb' else i % 7 if kind == 'edges' else i % 3 if kind == 'under' else i % 4
    if kind == 'climb':                # mixed waves: climbers beside gentle, flat and falling rows
        slope[:] = np.choose(j, [CLIMB, GENTLE1, GENTLE2, 0, DESCEND])
    elif kind == 'under':              # whole waves just under the threshold (and flat rows, which never trigger)
        slope[:] = np.where(j < 2, UNDER, 0)
    elif kind == 'edges':              # maximum in the ragged last tile, or only in the first
        slope[:] = np.choose(j, [0, 0, DESCEND, CLIMB, GENTLE1, 0, GENTLE1])
        last[:] = np.choose(j, [10 * _NAT, 0, 0, 0, 5 * _NAT, 0, 0])
        first[:] = np.choose(j, [0, 10 * _NAT, 0, 0, 0, 0, 25 * _NAT])
    else:                              # masked: climbers whose top tiles are hidden, rows whose first tiles are hidden
        slope[:] = np.choose(j, [CLIMB, CLIMB, GENTLE2, DESCEND])
    return slope, last, first


def lazy_problem(b, h, hkv, sq, skv, d, seed, masked):
    """Constructions A (tests/test_gpu_attn_range.py): plane (b, h) is kind LAZY_KINDS[h % 4].  q and k hold small
    integers, so every q.k is exact in float32; the scaled score of row i, key j (LAZY_SCALE) is

        slope_i (t_j - t_c) + intercept_i + last_i [j in the last tile] + first_i [j in the first tile]
        + bump_i [(i + j) % 4 == 0] + noise_ij            (raw units; t_j = j // 32, t_c the middle tile)

    with |noise| of a few raw units.  ``masked``: the plane of kind 'masked' hides, per row, the keys that carry the bump
    (its largest scores), plus the two top tiles (climbing rows) or the first 1 - 3 tiles; the other planes see every
    key.  Returns q, k, v, dctx, scale, mask (None unless ``masked``)."""
    assert d >= 16 and h % 4 == 0 and skv > 3 * TILE
    rng = np.random.default_rng(seed)
    nt = (skv + TILE - 1) // TILE
    jj = np.arange(skv)
    t = jj // TILE
    k = np.zeros([b, skv, hkv, d], dtype=np.float32)
    k[..., 0] = (t - (nt - 1) // 2)[None, :, None]
    k[..., 1] = 1.0
    k[..., 2] = (t == nt - 1)[None, :, None]
    k[..., 3] = (t == 0)[None, :, None]
    for u in range(4):
        k[..., 4 + u] = (jj % 4 == u)[None, :, None]
    k[..., 8:] = rng.integers(-1, 2, size=[b, skv, hkv, d - 8])
    q = np.zeros([b, sq, h, d], dtype=np.float32)
    ii = np.arange(sq)
    mask = np.ones([b, h, sq, skv], dtype=bool) if masked else None
    for bi in range(b):
        for hi in range(h):
            kind = LAZY_KINDS[hi % 4]
            slope, last, first = _slopes(kind, ii, bi)
            q[bi, :, hi, 0] = slope
            q[bi, :, hi, 1] = ((ii * 7 + bi) % 7 - 3) * 32                   # intercept: +-1.5 natural units
            q[bi, :, hi, 2] = last
            q[bi, :, hi, 3] = first
            if kind == 'masked':
                q[bi, ii, hi, 4 + (-ii) % 4] = 8 * _NAT                       # +8 natural units where (i + j) % 4 == 0
                if masked:
                    mk = mask[bi, hi]
                    mk[(ii[:, None] + jj[None, :]) % 4 == 0] = False
                    top = (ii % 4 == 0)[:, None] & (t >= nt - 2)[None, :]    # climbers: the two top tiles hidden
                    lead = (ii % 4 != 0)[:, None] & (t[None, :] < 1 + (ii[:, None] % 3))  # the first 1 - 3 tiles hidden
                    mk[top | lead] = False
            q[bi, :, hi, 8:] = rng.integers(-1, 2, size=[sq, d - 8])
    v = rng.standard_normal([b, skv, hkv, d]).astype(np.float32)
    dctx = rng.standard_normal([b, sq, h, d]).astype(np.float32)
    return q, k, v, dctx, LAZY_SCALE, mask


def plane_scores_log2(q, k, scale, bi, hi, mask=None):
    """Scaled scores of plane (bi, hi) in log2 units, masked positions -inf."""
    hkv = k.shape[2]
    s = scale * (q[bi, :, hi].astype(np.float64) @ k[bi, :, hi % hkv].astype(np.float64).T) * LOG2E
    if mask is not None:
        s = np.where(np.broadcast_to(mask, (q.shape[0], q.shape[2]) + s.shape)[bi, hi], s, -np.inf)
    return s


# ---- magnitude and shift -------------------------------------------------------------------------------------------
def shift_problem(b, h, hkv, sq, skv, d, seed, reach=200.0):
    """q, k, v, dctx (N(0,1); k on a grid of 2^-12) and a shift u per (b, K / V head) on a grid of 2^-4 with
    |u| < 2^11, so that k + u is exact in float32.  Row i of query head h then has every score moved by
    scale q_i . u[b, h % Hkv] -- up to ``reach`` natural units either way.  Returns q, k, v, dctx, scale, k + u, shift [B, Hq, Sq]."""
    rng = np.random.default_rng(seed)
    scale = 1.0 / np.sqrt(d)
    q = rng.standard_normal([b, sq, h, d]).astype(np.float32)
    k = (np.round(rng.standard_normal([b, skv, hkv, d]) * 4096) / 4096).astype(np.float32)
    v = rng.standard_normal([b, skv, hkv, d]).astype(np.float32)
    dctx = rng.standard_normal([b, sq, h, d]).astype(np.float32)
    u = rng.standard_normal([b, hkv, d])
    proj = np.stack([np.einsum('bqd,bd->bq', q[:, :, hi].astype(np.float64), u[:, hi % hkv]) for hi in range(h)], axis=1)
    u *= reach / (scale * np.abs(proj).max())
    u = np.round(u * 16) / 16
    assert np.abs(u).max() < 2048
    ku = (k.astype(np.float64) + u[:, None]).astype(np.float32)
    assert np.array_equal(ku.astype(np.float64), k.astype(np.float64) + u[:, None])
    shift = scale * np.stack([np.einsum('bqd,bd->bq', q[:, :, hi].astype(np.float64), u[:, hi % hkv]) for hi in range(h)], axis=1)
    return q, k, v, dctx, scale, ku, shift


def saturated_problem(b, h, hkv, sq, skv, d, seed, spread=30.0):
    """N(0,1) data with q scaled so that the scaled scores have standard deviation ``spread``: a softmax that is nearly
    one-hot in most rows."""
    rng = np.random.default_rng(seed)
    scale = 1.0 / np.sqrt(d)
    q = (rng.standard_normal([b, sq, h, d]) * spread).astype(np.float32)
    k, v = (rng.standard_normal([b, skv, hkv, d]).astype(np.float32) for _ in range(2))
    dctx = rng.standard_normal([b, sq, h, d]).astype(np.float32)
    return q, k, v, dctx, scale


def float32_reference(q, k, v, dctx, scale):
    """The reference's formulas evaluated in float32 (no mask, Hkv = Hq): what the bound must admit."""
    f = np.float32
    s = f(scale) * np.einsum('bqhd,bkhd->bhqk', q, k)
    top = s.max(axis=-1, keepdims=True)
    e = np.exp(s - top)
    tot = e.sum(axis=-1, keepdims=True)
    p = e / tot
    ctx = np.einsum('bhqk,bkhd->bqhd', p, v)
    dp = np.einsum('bqhd,bkhd->bhqk', dctx, v)
    ds = p * (dp - (p * dp).sum(axis=-1, keepdims=True)) * f(scale)
    return dict(ctx=ctx, lse=(top + np.log(tot))[..., 0], dq=np.einsum('bhqk,bkhd->bqhd', ds, k),
                dk=np.einsum('bhqk,bqhd->bkhd', ds, q), dv=np.einsum('bhqk,bqhd->bkhd', p, dctx))


# ---- masks -----------------------------------------------------------------------------------------------------------
PAD_LENGTHS = (700, 384, 300, 129)


def key_padding_mask(lengths, skv):
    """[B, 1, 1, Skv]: key j of batch b visible iff j < lengths[b]."""
    return (np.arange(skv)[None, :] < np.asarray(lengths)[:, None])[:, None, None, :]


def gap_mask(s):
    """Causal [1, 1, S, S], except that rows i % 5 == 0 see only the last 32 keys (at S = 2048: tile 63 alone): after a
    long gap for the late rows, ahead of the diagonal for the early ones."""
    i, j = np.arange(s)[:, None], np.arange(s)[None, :]
    last = j >= s - TILE
    return np.where(i % 5 == 0, last, j <= i)[None, None]
